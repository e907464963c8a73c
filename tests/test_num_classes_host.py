"""Host-side checks of the head's class count (1 .. 32): the limit is refused naming the value before anything is
packed or launched, configs.head_cfg(num_classes=) sets the head's count and the coder's modulus, and the state dict
has the shapes of the reference's.  CPU."""
import pytest

from transcar_amd import _lib as L, configs, synth


@pytest.mark.parametrize('bad', [0, 33, -1, 64, True, 23.0, '23', None])
def test_check_num_classes_refuses_naming_the_value(bad):
    with pytest.raises(L.TransCARHipError) as e:
        L.check_num_classes(bad)
    assert 'num_classes=%r is not supported' % (bad,) in str(e.value)


@pytest.mark.parametrize('ok', [1, 10, 16, 17, 23, 32])
def test_check_num_classes_accepts(ok):
    L.check_num_classes(ok)
    assert L.TC_MAX_CLASSES == 32


def test_head_cfg_sets_the_head_and_the_coder():
    cfg = configs.head_cfg(num_classes=23)
    assert cfg['num_classes'] == 23 and cfg['bbox_coder']['num_classes'] == 23
    assert configs.pts_bbox_head['num_classes'] == 10 and configs.pts_bbox_head['bbox_coder']['num_classes'] == 10
    assert configs.head_cfg() == configs.head_cfg(num_classes=None)
    with pytest.raises(L.TransCARHipError, match='num_classes=33'):
        configs.head_cfg(num_classes=33)
    with pytest.raises(L.TransCARHipError, match='num_classes=0'):
        configs.head_cfg(num_classes=0)


def test_state_dict_shapes():
    sd10, sd23 = synth.make_state_dict(seed=3), synth.make_state_dict(seed=3, num_classes=23)
    assert set(sd10) == set(sd23)
    wide = {k for k in sd23 if sd23[k].shape != sd10[k].shape}
    want = {'%s.6.%s' % (b, p) for b in ['cls_branches.%d' % i for i in range(6)] + ['final_cls', 'final_cls2', 'final_cls3']
            for p in ('weight', 'bias')}
    assert wide == want
    for k in wide:
        assert sd23[k].shape == ((23, 256) if k.endswith('weight') else (23,)), k


def test_built_head_carries_the_count_and_refuses_beyond_the_limit():
    import transcar_amd as T
    h = T.build_head(configs.head_cfg(num_classes=23))
    assert h.num_classes == 23 and h.cls_out_channels == 23 and h.bbox_coder.num_classes == 23
    assert {k: tuple(v.shape) for k, v in h.state_dict().items()} == \
        {k: tuple(v.shape) for k, v in synth.make_state_dict(seed=3, num_classes=23).items()}
    assert h.weights_struct().num_classes == 23 and h.decoder_heads_struct().num_classes == 23
    cfg = configs.head_cfg()
    cfg['num_classes'] = 33                     # past head_cfg's own check: the module's structs refuse
    h = T.build_head(cfg)
    with pytest.raises(L.TransCARHipError, match='num_classes=33'):
        h.weights_struct()
    with pytest.raises(L.TransCARHipError, match='num_classes=33'):
        h.decoder_heads_struct()
