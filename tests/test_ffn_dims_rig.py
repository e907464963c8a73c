"""ffn_dims_rig.py's committed radar seeds on the CPU: on each head's frame the oracle's closest gate decision sits at
least MIN_MARGIN from its radius, so that the gate rows the GPU tests set apart (MAX_GATE_ROWS) only have to cover the
kernels' rounding.  No GPU."""
import pytest

import ffn_dims_rig as FR


@pytest.mark.parametrize('F,refine', sorted(FR.SEEDS))
def test_committed_seed_keeps_the_gates_off_their_radii(F, refine):
    m = FR.margin(F, refine)
    print('feedforward_channels=%d with_box_refine=%s seed %d: margin %.3e m' % (F, refine, FR.SEEDS[F, refine], m))
    assert m >= FR.MIN_MARGIN
