"""The rig of the head's configuration keys taken together: a pairwise (2-way) covering set of head configurations on the
tiny maps -- every admissible pair of values of two axes stands in some row -- for the forward (INFERENCE_ROWS) and for one
training iteration (TRAINING_ROWS), the greedy generator that produced the two tables, one radar frame per row and sample
chosen by the gate-margin search, and one oracle driver, oracle_row.

The other rigs each serve one axis and keep every other key at the TransCAR configs' value.  Here a row carries all of
them: `variant(row)` spells the row as a head_variant_rig variant, through which the head is built and the oracle told every
key by argument, and the oracle is fed the [n, F] rows the row's filter range keeps.  The builders, checkers, tolerances and
the gate-margin discipline are head_variant_rig's and radar_input_rig's, as they are.

A row is a dict of axis -> value; gate, filter range and geometry are spelled as names (GATES, RANGES, GEOMS), the chain path
as num_cams_rig.PATHS spells it (and 'unfused').  A training row fixes its decoder-side keys by name (DECODERS).  What is
computed on the CPU is computed once per row and sample and kept."""
import itertools

import numpy as np
import torch

import head_variant_rig as R
import num_cams_rig as NR
import radar_heads_rig as RR
import radar_input_rig as RI
from oracle import transcar_oracle as O
from radar_input_rig import BACKWARDS, FACE_RANGE
from transcar_amd import synth

# ---- the axes ---------------------------------------------------------------------------------------------------------------
INFERENCE_AXES = dict(
    num_cams=(1, 6, 9, 16), num_levels=(1, 2, 4), num_points=(1, 3, 5), with_box_refine=(True, False),
    num_heads=(4, 8, 16), radar_num_heads=(4, 8, 16), num_classes=(1, 10, 17, 32), num_query=(37, 72),
    num_fusion_layers=(1, 2, 3), radar_gate=('default', 'circle', 'wide3'), radar_num_tokens=(64, 1500, 2048),
    radar_in_dims=(4, 36, 64), radar_point_range=('default', 'face'), geometry=('default', 'geom'), samples=(1, 2),
    path=('f32-4', 'f32-8', 'f32-16', 'f16x2-16', 'f16x2-32', 'unfused'), outputs=('fusion', 'all'))
TRAINING_AXES = dict(
    radar_num_heads=(4, 8, 16), num_classes=(1, 10, 17, 32), num_query=(37, 72), num_fusion_layers=(1, 2, 3),
    radar_gate=('default', 'circle', 'wide3'), radar_num_tokens=(64, 1500, 2048), radar_in_dims=(4, 36, 64),
    radar_point_range=('default', 'face'), backward=('chain', 'operators', 'deterministic'), dropout=(0.0, 0.1),
    decoder=('five-norefine', 'twelve-by-two'))
MAX_INFERENCE_ROWS, MAX_TRAINING_ROWS = 36, 24
GATES = {'default': None, 'circle': R.CIRCLE, 'wide3': R.WIDE3}
RANGES = {'default': None, 'face': FACE_RANGE}
GEOMS = {'default': None, 'geom': R.GEOM}
PATHS = dict({k: v for k, v in NR.PATHS.items() if k != 'auto'}, unfused=dict(unfused=True))
# the decoder under a training row (frozen): neither is the configs', one has more than 8 cameras
DECODERS = {'five-norefine': dict(num_cams=5, num_levels=4, num_points=1, with_box_refine=False, num_heads=16),
            'twelve-by-two': dict(num_cams=12, num_levels=2, num_points=3, with_box_refine=True, num_heads=4)}
# the value a key has when a head is built without it
DEFAULTS = dict(num_cams=6, num_levels=4, num_points=1, with_box_refine=True, num_heads=8, radar_num_heads=8, num_classes=10,
                num_fusion_layers=3, radar_gate='default', radar_num_tokens=1500, radar_in_dims=36, radar_point_range='default',
                geometry='default')
assert set(BACKWARDS) == set(TRAINING_AXES['backward']) and set(PATHS) == set(INFERENCE_AXES['path'])


def cam_logits_ok(num_cams, num_levels, num_points):
    """TC_MAX_CAM_LOGITS, the only joint constraint"""
    from transcar_amd._lib import TC_MAX_CAM_LOGITS
    return num_cams * num_levels * num_points <= TC_MAX_CAM_LOGITS


def unconstrained():
    return True


# ---- the generator -----------------------------------------------------------------------------------------------------------
def admissible_pairs(axes, ok):
    """{((axis, value), (axis, value))}: the pairs of values of two axes that some full row satisfying `ok` contains."""
    names = list(axes)
    constrained = [a for a in names if a in ok.__code__.co_varnames[:ok.__code__.co_argcount]]
    pairs = set()
    for a, b in itertools.combinations(names, 2):
        free = [c for c in constrained if c not in (a, b)]
        for va in axes[a]:
            for vb in axes[b]:
                fixed = {a: va, b: vb}
                if any(ok(**{c: dict(fixed, **dict(zip(free, vs))).get(c) for c in constrained})
                       for vs in itertools.product(*(axes[c] for c in free))):
                    pairs.add(((a, va), (b, vb)))
    return pairs


def covered(row, names):
    return {((a, row[a]), (b, row[b])) for a, b in itertools.combinations(names, 2)}


def generate(axes, ok, tries=64, seed=1):
    """Greedy pairwise rows: each row is the best of `tries` candidates, a candidate being grown from an uncovered pair
    by giving the other axes, in an order a fixed linear congruential sequence draws, the value that covers the most
    still uncovered pairs with the axes already set (ties: the first value)."""
    names = list(axes)
    constrained = [a for a in names if a in ok.__code__.co_varnames[:ok.__code__.co_argcount]]
    todo = admissible_pairs(axes, ok)
    state = [seed]

    def draw(n):
        state[0] = (state[0] * 1103515245 + 12345) % 2 ** 31
        return (state[0] >> 8) % n

    def feasible(row):
        free = [c for c in constrained if c not in row]
        return any(ok(**dict({c: row[c] for c in constrained if c in row}, **dict(zip(free, vs))))
                   for vs in itertools.product(*(axes[c] for c in free)))

    rows = []
    while todo:
        best = None
        start = sorted(todo, key=repr)
        for t in range(tries):
            (a, va), (b, vb) = start[draw(len(start))]
            row = {a: va, b: vb}
            rest = [n for n in names if n not in row]
            for i in range(len(rest) - 1, 0, -1):
                j = draw(i + 1)
                rest[i], rest[j] = rest[j], rest[i]
            for n in rest:
                gains = []
                for v in axes[n]:
                    if not feasible(dict(row, **{n: v})):
                        continue
                    gains.append((sum(((min((n, v), (m, row[m]), key=lambda p: names.index(p[0])),
                                        max((n, v), (m, row[m]), key=lambda p: names.index(p[0]))) in todo) for m in row), v))
                row[n] = max(gains, key=lambda g: g[0])[1]
            gain = len(covered(row, names) & todo)
            if best is None or gain > best[0]:
                best = (gain, row)
        rows.append({n: best[1][n] for n in names})
        todo -= covered(best[1], names)
    return rows


INFERENCE_SEED, TRAINING_SEED = 4, 6          # of generate's seeds 1 .. 6 those with the fewest rows

INFERENCE_ROWS = [
    dict(num_cams=1, num_levels=1, num_points=1, with_box_refine=True, num_heads=16, radar_num_heads=4,
         num_classes=1, num_query=37, num_fusion_layers=3, radar_gate='default', radar_num_tokens=64,
         radar_in_dims=4, radar_point_range='default', geometry='default', samples=1, path='f32-4',
         outputs='fusion'),
    dict(num_cams=6, num_levels=2, num_points=3, with_box_refine=False, num_heads=4, radar_num_heads=8,
         num_classes=10, num_query=72, num_fusion_layers=1, radar_gate='circle', radar_num_tokens=1500,
         radar_in_dims=36, radar_point_range='face', geometry='geom', samples=2, path='f32-4', outputs='all'),
    dict(num_cams=9, num_levels=4, num_points=5, with_box_refine=True, num_heads=8, radar_num_heads=16,
         num_classes=17, num_query=72, num_fusion_layers=2, radar_gate='wide3', radar_num_tokens=2048,
         radar_in_dims=64, radar_point_range='face', geometry='default', samples=2, path='f32-8', outputs='fusion'),
    dict(num_cams=16, num_levels=4, num_points=3, with_box_refine=False, num_heads=8, radar_num_heads=4,
         num_classes=32, num_query=37, num_fusion_layers=2, radar_gate='circle', radar_num_tokens=2048,
         radar_in_dims=4, radar_point_range='default', geometry='geom', samples=1, path='f32-16', outputs='all'),
    dict(num_cams=9, num_levels=1, num_points=5, with_box_refine=False, num_heads=4, radar_num_heads=16,
         num_classes=1, num_query=37, num_fusion_layers=3, radar_gate='wide3', radar_num_tokens=1500,
         radar_in_dims=64, radar_point_range='default', geometry='geom', samples=1, path='f16x2-16', outputs='all'),
    dict(num_cams=16, num_levels=1, num_points=1, with_box_refine=True, num_heads=16, radar_num_heads=8,
         num_classes=32, num_query=72, num_fusion_layers=1, radar_gate='default', radar_num_tokens=64,
         radar_in_dims=36, radar_point_range='face', geometry='geom', samples=2, path='f16x2-32', outputs='fusion'),
    dict(num_cams=6, num_levels=2, num_points=3, with_box_refine=False, num_heads=16, radar_num_heads=16,
         num_classes=17, num_query=37, num_fusion_layers=1, radar_gate='default', radar_num_tokens=64,
         radar_in_dims=64, radar_point_range='default', geometry='default', samples=1, path='unfused',
         outputs='all'),
    dict(num_cams=6, num_levels=2, num_points=1, with_box_refine=True, num_heads=4, radar_num_heads=4,
         num_classes=10, num_query=72, num_fusion_layers=3, radar_gate='wide3', radar_num_tokens=1500,
         radar_in_dims=4, radar_point_range='face', geometry='default', samples=2, path='f32-16', outputs='fusion'),
    dict(num_cams=1, num_levels=4, num_points=1, with_box_refine=False, num_heads=8, radar_num_heads=8,
         num_classes=1, num_query=37, num_fusion_layers=3, radar_gate='circle', radar_num_tokens=2048,
         radar_in_dims=36, radar_point_range='face', geometry='default', samples=1, path='unfused',
         outputs='fusion'),
    dict(num_cams=1, num_levels=4, num_points=5, with_box_refine=True, num_heads=4, radar_num_heads=8,
         num_classes=10, num_query=72, num_fusion_layers=2, radar_gate='default', radar_num_tokens=1500,
         radar_in_dims=36, radar_point_range='default', geometry='geom', samples=1, path='f32-8', outputs='all'),
    dict(num_cams=9, num_levels=4, num_points=5, with_box_refine=True, num_heads=16, radar_num_heads=4,
         num_classes=10, num_query=37, num_fusion_layers=1, radar_gate='circle', radar_num_tokens=64,
         radar_in_dims=4, radar_point_range='default', geometry='default', samples=2, path='f16x2-16',
         outputs='fusion'),
    dict(num_cams=6, num_levels=1, num_points=1, with_box_refine=False, num_heads=8, radar_num_heads=16,
         num_classes=10, num_query=37, num_fusion_layers=2, radar_gate='circle', radar_num_tokens=2048,
         radar_in_dims=64, radar_point_range='default', geometry='default', samples=1, path='f16x2-32',
         outputs='all'),
    dict(num_cams=1, num_levels=2, num_points=3, with_box_refine=True, num_heads=8, radar_num_heads=16,
         num_classes=1, num_query=72, num_fusion_layers=1, radar_gate='wide3', radar_num_tokens=2048,
         radar_in_dims=36, radar_point_range='face', geometry='default', samples=2, path='f16x2-16',
         outputs='fusion'),
    dict(num_cams=16, num_levels=2, num_points=5, with_box_refine=True, num_heads=4, radar_num_heads=16,
         num_classes=32, num_query=72, num_fusion_layers=2, radar_gate='wide3', radar_num_tokens=64, radar_in_dims=4,
         radar_point_range='default', geometry='default', samples=2, path='unfused', outputs='fusion'),
    dict(num_cams=16, num_levels=1, num_points=1, with_box_refine=False, num_heads=16, radar_num_heads=4,
         num_classes=17, num_query=37, num_fusion_layers=3, radar_gate='circle', radar_num_tokens=1500,
         radar_in_dims=4, radar_point_range='default', geometry='geom', samples=1, path='f32-8', outputs='fusion'),
    dict(num_cams=9, num_levels=1, num_points=3, with_box_refine=True, num_heads=8, radar_num_heads=8,
         num_classes=17, num_query=37, num_fusion_layers=1, radar_gate='default', radar_num_tokens=64,
         radar_in_dims=36, radar_point_range='default', geometry='default', samples=1, path='f32-16',
         outputs='fusion'),
    dict(num_cams=6, num_levels=4, num_points=5, with_box_refine=True, num_heads=16, radar_num_heads=8,
         num_classes=32, num_query=37, num_fusion_layers=2, radar_gate='wide3', radar_num_tokens=2048,
         radar_in_dims=64, radar_point_range='default', geometry='default', samples=1, path='f32-4',
         outputs='fusion'),
    dict(num_cams=1, num_levels=2, num_points=3, with_box_refine=True, num_heads=4, radar_num_heads=4,
         num_classes=17, num_query=37, num_fusion_layers=3, radar_gate='wide3', radar_num_tokens=1500,
         radar_in_dims=64, radar_point_range='default', geometry='default', samples=1, path='f16x2-32',
         outputs='fusion'),
    dict(num_cams=9, num_levels=2, num_points=1, with_box_refine=True, num_heads=4, radar_num_heads=8,
         num_classes=32, num_query=37, num_fusion_layers=3, radar_gate='default', radar_num_tokens=2048,
         radar_in_dims=4, radar_point_range='default', geometry='default', samples=1, path='f16x2-16',
         outputs='fusion'),
    dict(num_cams=9, num_levels=1, num_points=1, with_box_refine=True, num_heads=8, radar_num_heads=4,
         num_classes=10, num_query=37, num_fusion_layers=1, radar_gate='default', radar_num_tokens=1500,
         radar_in_dims=36, radar_point_range='default', geometry='geom', samples=1, path='unfused',
         outputs='fusion'),
    dict(num_cams=16, num_levels=1, num_points=5, with_box_refine=True, num_heads=16, radar_num_heads=16,
         num_classes=1, num_query=37, num_fusion_layers=2, radar_gate='default', radar_num_tokens=64,
         radar_in_dims=64, radar_point_range='default', geometry='default', samples=1, path='f32-16',
         outputs='fusion'),
    dict(num_cams=6, num_levels=2, num_points=3, with_box_refine=True, num_heads=4, radar_num_heads=4, num_classes=1,
         num_query=37, num_fusion_layers=1, radar_gate='default', radar_num_tokens=64, radar_in_dims=4,
         radar_point_range='default', geometry='default', samples=1, path='f32-8', outputs='fusion'),
    dict(num_cams=9, num_levels=4, num_points=5, with_box_refine=True, num_heads=4, radar_num_heads=4, num_classes=1,
         num_query=37, num_fusion_layers=1, radar_gate='default', radar_num_tokens=64, radar_in_dims=4,
         radar_point_range='default', geometry='default', samples=1, path='f16x2-32', outputs='fusion'),
    dict(num_cams=16, num_levels=1, num_points=1, with_box_refine=True, num_heads=8, radar_num_heads=16,
         num_classes=10, num_query=37, num_fusion_layers=1, radar_gate='default', radar_num_tokens=64,
         radar_in_dims=4, radar_point_range='default', geometry='default', samples=1, path='f32-4',
         outputs='fusion'),
    dict(num_cams=6, num_levels=1, num_points=1, with_box_refine=True, num_heads=4, radar_num_heads=4,
         num_classes=17, num_query=37, num_fusion_layers=2, radar_gate='default', radar_num_tokens=64,
         radar_in_dims=4, radar_point_range='default', geometry='default', samples=1, path='f16x2-16',
         outputs='fusion'),
    dict(num_cams=1, num_levels=1, num_points=1, with_box_refine=True, num_heads=4, radar_num_heads=4,
         num_classes=32, num_query=37, num_fusion_layers=1, radar_gate='default', radar_num_tokens=1500,
         radar_in_dims=4, radar_point_range='default', geometry='default', samples=1, path='f32-8',
         outputs='fusion'),
    dict(num_cams=9, num_levels=1, num_points=1, with_box_refine=True, num_heads=4, radar_num_heads=4,
         num_classes=17, num_query=37, num_fusion_layers=1, radar_gate='default', radar_num_tokens=64,
         radar_in_dims=4, radar_point_range='default', geometry='default', samples=1, path='f32-4',
         outputs='fusion'),
    dict(num_cams=1, num_levels=1, num_points=1, with_box_refine=True, num_heads=4, radar_num_heads=4, num_classes=1,
         num_query=37, num_fusion_layers=1, radar_gate='default', radar_num_tokens=64, radar_in_dims=4,
         radar_point_range='default', geometry='default', samples=1, path='f32-16', outputs='fusion'),
    dict(num_cams=16, num_levels=1, num_points=1, with_box_refine=True, num_heads=4, radar_num_heads=4,
         num_classes=1, num_query=37, num_fusion_layers=1, radar_gate='default', radar_num_tokens=64,
         radar_in_dims=4, radar_point_range='default', geometry='default', samples=1, path='f16x2-16',
         outputs='fusion'),
]
TRAINING_ROWS = [
    dict(radar_num_heads=4, num_classes=1, num_query=37, num_fusion_layers=1, radar_gate='default',
         radar_num_tokens=64, radar_in_dims=4, radar_point_range='default', backward='chain', dropout=0.1,
         decoder='five-norefine'),
    dict(radar_num_heads=8, num_classes=10, num_query=72, num_fusion_layers=2, radar_gate='circle',
         radar_num_tokens=1500, radar_in_dims=36, radar_point_range='face', backward='chain', dropout=0.0,
         decoder='twelve-by-two'),
    dict(radar_num_heads=16, num_classes=32, num_query=72, num_fusion_layers=3, radar_gate='wide3',
         radar_num_tokens=2048, radar_in_dims=64, radar_point_range='default', backward='operators', dropout=0.0,
         decoder='five-norefine'),
    dict(radar_num_heads=16, num_classes=17, num_query=37, num_fusion_layers=3, radar_gate='default',
         radar_num_tokens=1500, radar_in_dims=64, radar_point_range='face', backward='deterministic', dropout=0.1,
         decoder='twelve-by-two'),
    dict(radar_num_heads=8, num_classes=1, num_query=37, num_fusion_layers=2, radar_gate='wide3',
         radar_num_tokens=2048, radar_in_dims=4, radar_point_range='face', backward='operators', dropout=0.1,
         decoder='twelve-by-two'),
    dict(radar_num_heads=4, num_classes=17, num_query=72, num_fusion_layers=2, radar_gate='circle',
         radar_num_tokens=64, radar_in_dims=36, radar_point_range='default', backward='deterministic', dropout=0.0,
         decoder='five-norefine'),
    dict(radar_num_heads=4, num_classes=32, num_query=37, num_fusion_layers=1, radar_gate='circle',
         radar_num_tokens=1500, radar_in_dims=36, radar_point_range='face', backward='operators', dropout=0.1,
         decoder='twelve-by-two'),
    dict(radar_num_heads=8, num_classes=10, num_query=72, num_fusion_layers=1, radar_gate='default',
         radar_num_tokens=2048, radar_in_dims=4, radar_point_range='default', backward='deterministic', dropout=0.0,
         decoder='five-norefine'),
    dict(radar_num_heads=4, num_classes=10, num_query=37, num_fusion_layers=3, radar_gate='wide3',
         radar_num_tokens=64, radar_in_dims=64, radar_point_range='default', backward='chain', dropout=0.0,
         decoder='twelve-by-two'),
    dict(radar_num_heads=16, num_classes=1, num_query=72, num_fusion_layers=3, radar_gate='circle',
         radar_num_tokens=1500, radar_in_dims=4, radar_point_range='default', backward='chain', dropout=0.0,
         decoder='five-norefine'),
    dict(radar_num_heads=16, num_classes=10, num_query=72, num_fusion_layers=2, radar_gate='default',
         radar_num_tokens=64, radar_in_dims=36, radar_point_range='face', backward='operators', dropout=0.1,
         decoder='five-norefine'),
    dict(radar_num_heads=4, num_classes=17, num_query=37, num_fusion_layers=1, radar_gate='wide3',
         radar_num_tokens=2048, radar_in_dims=36, radar_point_range='default', backward='chain', dropout=0.0,
         decoder='five-norefine'),
    dict(radar_num_heads=8, num_classes=32, num_query=37, num_fusion_layers=2, radar_gate='default',
         radar_num_tokens=64, radar_in_dims=64, radar_point_range='default', backward='chain', dropout=0.0,
         decoder='five-norefine'),
    dict(radar_num_heads=8, num_classes=1, num_query=37, num_fusion_layers=3, radar_gate='wide3',
         radar_num_tokens=1500, radar_in_dims=36, radar_point_range='default', backward='deterministic', dropout=0.0,
         decoder='five-norefine'),
    dict(radar_num_heads=16, num_classes=1, num_query=37, num_fusion_layers=1, radar_gate='circle',
         radar_num_tokens=2048, radar_in_dims=64, radar_point_range='default', backward='chain', dropout=0.0,
         decoder='five-norefine'),
    dict(radar_num_heads=8, num_classes=17, num_query=37, num_fusion_layers=1, radar_gate='default',
         radar_num_tokens=64, radar_in_dims=4, radar_point_range='default', backward='operators', dropout=0.0,
         decoder='five-norefine'),
    dict(radar_num_heads=4, num_classes=32, num_query=37, num_fusion_layers=1, radar_gate='default',
         radar_num_tokens=64, radar_in_dims=4, radar_point_range='default', backward='deterministic', dropout=0.0,
         decoder='five-norefine'),
]


def full(row):
    """A row with every key of an inference row: a training row's decoder spelled out, one sample, the configs' geometry."""
    if 'decoder' not in row:
        return row
    return dict(row, geometry='default', samples=1, **DECODERS[row['decoder']])


def row_id(row):
    """The non-default keys of a row, spelled for a test id."""
    row, parts = full(row), []
    short = dict(num_cams='cams', num_levels='L', num_points='P', num_heads='h', radar_num_heads='rh', num_classes='c',
                 num_fusion_layers='fl', radar_num_tokens='t', radar_in_dims='F')
    for k, tag in short.items():
        if row[k] != DEFAULTS[k]:
            parts.append('%s%d' % (tag, row[k]))
    parts.append('q%d' % row['num_query'])
    if not row['with_box_refine']:
        parts.append('norefine')
    parts += [row[k] for k in ('radar_gate', 'radar_point_range', 'geometry') if row[k] != 'default']
    if row['samples'] == 2:
        parts.append('b2')
    parts += ['%s' % row[k] for k in ('path', 'outputs', 'backward') if k in row and row[k] != 'fusion']
    if row.get('dropout'):
        parts.append('drop')
    return '-'.join(parts)


def non_default_keys(row):
    return sum(row[k] != v for k, v in DEFAULTS.items())


# ---- a row's head, weights and maps ----------------------------------------------------------------------------------------------
def ring(row, b=0):
    """the cameras of sample b: the row's ring over the row's base geometry; a second sample has the mounts moved"""
    row = full(row)
    return NR.Ring(row['num_cams'], NR.JITTER if b else None, GEOMS[row['geometry']])


def variant(row, b=0):
    """head_variant_rig's variant of the row: every configuration key of the row, and sample b's cameras as the geometry"""
    row = full(row)
    kw = {k: row[k] for k in ('num_levels', 'num_points', 'with_box_refine', 'num_heads', 'num_classes', 'num_query',
                              'num_fusion_layers', 'radar_num_heads', 'radar_num_tokens', 'radar_in_dims')}
    return dict(kw, radar_gate=GATES[row['radar_gate']], radar_point_range=RANGES[row['radar_point_range']], geometry=ring(row, b))


def feats(row):
    """the row's maps [samples, N, C, H, W], the first num_levels tiny levels"""
    row = full(row)
    return NR.feats(row['num_cams'], batch=row['samples'], num_levels=row['num_levels'])


# ---- the oracle under a row ----------------------------------------------------------------------------------------------------
_SD, _TRACE, _ROWS, _ORACLE, _FP64 = {}, {}, {}, {}, {}
DECODER_KEYS = ('num_cams', 'num_levels', 'num_points', 'with_box_refine', 'num_heads', 'num_classes', 'num_query', 'geometry', 'samples')


def _key(row):
    return tuple(sorted(full(row).items()))


def oracle_sd(row):
    """the row's weights as the oracle takes them (kept: a row's frames and checks share one dict)"""
    if _key(row) not in _SD:
        _SD[_key(row)] = O.to_torch_sd(R.state_dict(**variant(row)))
    return _SD[_key(row)]


def sample_feats(row, b):
    return [torch.from_numpy(f[b:b + 1]) for f in feats(row)]


def decoder_trace(row, b=0, double=False, sd=None):
    """O.transformer of sample b under the row, what head_forward takes as decoder_trace.  The decoder's weights are drawn
    before the fusion stack's and the radar encoder's: the trace is kept per decoder-side key set.  double: the fp64
    evaluation (weights, maps and cameras .double()).  sd: other weights than the row's (not kept)."""
    row = full(row)
    key = tuple(row[k] for k in DECODER_KEYS) + (b, double)
    if sd is not None or key not in _TRACE:
        geom, maps = ring(row, b), sample_feats(row, b)
        l2i = torch.from_numpy(geom.lidar2img()).float()[None]
        weights = oracle_sd(row) if sd is None else sd
        if double:
            weights, maps, l2i = {k: v.detach().double() for k, v in weights.items()}, [f.double() for f in maps], l2i.double()
        with torch.no_grad():
            trace = O.transformer(weights, maps, list(geom.pc_range), l2i, geom.hw, **R.decoder_kw(**variant(row, b)))
        if sd is not None:
            return trace
        _TRACE[key] = trace
    return _TRACE[key]


def head_forward(row, b, kept, trace=None, sd=None, **kw):
    """O.head_forward of sample b under the row on the rows `kept` (already filtered by the row's range); kw: its other
    arguments."""
    return R.oracle_forward(oracle_sd(row) if sd is None else sd, sample_feats(row, b), kept, variant(row, b),
                            decoder_trace=decoder_trace(row, b) if trace is None else trace, **kw)


def gate_centres(row, b=0):
    """[Q, 2] metres: the decoder's last reference points of sample b, where fusion layer 1 gates"""
    return O.denormalised_refs(decoder_trace(row, b)[2][-1], list(ring(row, b).pc_range))[0, :, :2].numpy().astype(np.float64)


# ---- frames ------------------------------------------------------------------------------------------------------------------------
# rows per frame by token count: more than 64 kept rows at 64 tokens (truncation), a T above 1500 at 2048; four times as
# many under FACE_RANGE, which keeps about a third of them
N_ROWS = {64: 150, 1500: 300, 2048: 1700}
SEED_RANGE = range(2, 80)


def frame_rows(row, b, seed):
    """-> ([n, F] float32 rows as the head gets them, the rows the row's filter range keeps): radar_input_rig.make_rows
    around sample b's own gate centres, two queries of three (the third gets no rows of its own: queries without a hit
    whatever the gate's radius)"""
    row = full(row)
    key = (tuple(row[k] for k in DECODER_KEYS), row['radar_num_tokens'], row['radar_in_dims'], row['radar_point_range'], b, seed)
    if key not in _ROWS:
        mult = 4 if row['radar_point_range'] == 'face' else 1
        cen = gate_centres(row, b)
        rows = RI.make_rows(seed, mult * N_ROWS[row['radar_num_tokens']], row['radar_in_dims'], near=mult * RI.NEAR,
                            centres=cen[np.arange(len(cen)) % 3 != 2])
        _ROWS[key] = rows, rows[RI.in_range(rows, RANGES[row['radar_point_range']] or RI.POINT_RANGE)]
    return _ROWS[key]


def gate_margin(row, b, seed):
    """metres between the oracle's closest gate decision on the frame of `seed` and its radius"""
    margins = []
    with torch.no_grad():
        head_forward(row, b, frame_rows(row, b, seed)[1], gate_probe=R.margin_probe(margins))
    assert len(margins) == full(row)['num_fusion_layers']
    return min(margins)


def search_seed(row, b=0):
    """-> (seed, margin): of SEED_RANGE the seed with the largest gate margin.  A training row's seed must also serve
    influential_ties (below): the ties set apart at most MAX_TIED less two to spare and the others below half of TIE_BOUND;
    where the best such seed is closer than radar_input_rig.MIN_MARGIN to a gate's radius, nothing is spared."""
    margins = {s: gate_margin(row, b, s) for s in SEED_RANGE}
    order = sorted(margins, key=margins.get, reverse=True)
    if 'decoder' not in row:
        return order[0], margins[order[0]]
    ties = {}
    for spare in (2, 0):
        for s in order:
            if margins[s] < RI.MIN_MARGIN and spare:
                break
            if s not in ties:
                ties[s] = influential_ties(row, seed=s)
            if len(ties[s][0]) <= MAX_TIED - spare and ties[s][1] < RR.TIE_BOUND / 2:
                return s, margins[s]
    raise AssertionError('no seed of %r serves' % (SEED_RANGE,))


# What a row with more than 8 cameras must show in every decoder layer (num_cams_rig.assert_coverage), per camera count.
# num_cams_rig.LEAST's counts are those of its own 72-query rig; a row's reference points are given by its seeded weights,
# 37 of them in most rows (at 9 cameras x 37 queries two or three queries see camera 8), so the floors are what the rows of
# a count show, the least over its rows, samples and layers: a later change of weights or geometry that shrinks the generic
# kernels' share is seen.
LEAST = {9: dict(high_only=0, low_and_high=1, either=2, three=0, last=2),
         12: dict(high_only=7, low_and_high=3, either=13, three=0, last=5),
         16: dict(high_only=9, low_and_high=0, either=19, three=17, last=1)}
# per row, one (seed, margin in metres) per sample: search_seed's result; tests/test_variant_pairs_host.py measures every
# margin again, holds it to radar_input_rig.MIN_MARGIN and repeats the search on some rows.
INFERENCE_FRAMES = [
    ((37, 9.050e-03),), ((47, 7.582e-02), (47, 7.582e-02),), ((7, 2.241e-03), (59, 2.230e-03),), ((20, 8.633e-02),),
    ((64, 2.599e-03),), ((49, 5.470e-02), (49, 6.123e-02),), ((29, 4.393e-02),), ((52, 1.633e-03), (2, 1.933e-03),),
    ((55, 1.158e-02),), ((39, 1.673e-02),), ((74, 4.591e-01), (5, 6.299e-01),), ((62, 2.045e-02),),
    ((46, 3.318e-03), (59, 2.549e-03),), ((58, 1.099e-02), (52, 1.419e-02),), ((43, 1.673e-02),), ((74, 4.547e-02),),
    ((46, 2.929e-03),), ((45, 1.924e-03),), ((41, 3.709e-03),), ((14, 1.640e-02),), ((52, 1.982e-02),),
    ((40, 4.559e-02),), ((54, 4.304e-02),), ((40, 4.611e-02),), ((70, 1.513e-02),), ((72, 2.497e-02),),
    ((54, 5.912e-02),), ((40, 4.921e-02),), ((54, 5.343e-02),),
]
TRAINING_FRAMES = [
    ((54, 4.496e-02),), ((76, 4.799e-02),), ((22, 1.170e-03),), ((60, 1.124e-03),), ((50, 1.201e-03),),
    ((48, 2.258e-01),), ((76, 1.199e-01),), ((18, 7.351e-03),), ((22, 6.457e-03),), ((59, 1.099e-02),),
    ((29, 2.234e-02),), ((22, 5.675e-03),), ((41, 2.265e-02),), ((43, 1.354e-03),), ((42, 5.611e-02),),
    ((54, 6.016e-02),), ((54, 5.653e-02),),
]


def frame_seed(row, b=0):
    if 'decoder' in row:
        return TRAINING_FRAMES[TRAINING_ROWS.index(row)][b]
    return INFERENCE_FRAMES[INFERENCE_ROWS.index(row)][b]


def oracle_row(row, b=0):
    """The oracle's head on sample b of the row's frame -> dict(sd, rows, kept, want, dbg, masks: the gate masks [Q, N] per
    layer (True = masked), margin: metres between the closest gate decision and its radius).  Kept per row and sample."""
    key = _key(row) + (b,)
    if key not in _ORACLE:
        rows, kept = frame_rows(row, b, frame_seed(row, b)[0])
        masks, margins = [], []
        with torch.no_grad():
            want, dbg = head_forward(row, b, kept, return_debug=True, gate_probe=R.margin_probe(margins, masks))
        assert dbg['fill_in'] == min(full(row)['radar_num_tokens'], len(kept))
        assert all(torch.equal((~m).sum(1), h) for m, h in zip(masks, dbg['hit_counts']))
        _ORACLE[key] = dict(sd=oracle_sd(row), rows=rows, kept=kept, want=want, dbg=dbg, masks=masks, margin=min(margins))
    return _ORACLE[key]


def oracle_fp64(row, b=0):
    """head_variant_rig.oracle_fp64_deviation under the row: the decoder evaluated in fp64 and the fusion stack on its
    states -> dict(hs_dev [Q], out_dev [Q], hit_counts: the gate decisions of that evaluation, per layer)."""
    key = _key(row) + (b,)
    if key not in _FP64:
        o = oracle_row(row, b)
        trace64 = decoder_trace(row, b, double=True)
        hs_dev = (o['dbg']['hs'].double() - trace64[0].permute(0, 2, 1, 3)).abs().amax(dim=(0, 1, 3))
        trace = tuple(t.float() if torch.is_tensor(t) else t for t in trace64)
        with torch.no_grad():
            outs64, dbg64 = head_forward(row, b, o['kept'], trace=trace, return_debug=True)
        out_dev = torch.stack([(o['want'][k] - outs64[k]).abs().amax(dim=(0, 1, 3)) for k in ('all_cls_scores', 'all_bbox_preds')]).amax(0)
        _FP64[key] = dict(hs_dev=hs_dev.numpy(), out_dev=out_dev.numpy(), hit_counts=dbg64['hit_counts'])
    return _FP64[key]


def oracle_with(row, b=0, **override):
    """The oracle's outputs on the row's frame and weights with some keys set to other values (a key the state dict's shapes
    do not depend on): what a kernel that ignored the key would be compared with."""
    other = dict(full(row), **override)
    o = oracle_row(row, b)
    kept = o['rows'][RI.in_range(o['rows'], RANGES[other['radar_point_range']] or RI.POINT_RANGE)]
    trace = decoder_trace(other, b, sd=o['sd'])
    with torch.no_grad():
        return head_forward(other, b, kept, trace=trace, sd=o['sd'])


# ---- training --------------------------------------------------------------------------------------------------------------------
SEED = 5                 # FusionTrainer(seed=)


def ground_truth(row):
    """G7's boxes drawn from the row's classes: (boxes [24, 9] bottom-centred, labels [24])"""
    return synth.make_gt(seed=7, n=24, num_classes=row['num_classes'])


def expected_gradients(row):
    """the tensors an iteration gives a gradient: the encoders' 14 and 28 per fusion layer"""
    return 14 + 28 * row['num_fusion_layers']


def dropout_masks(row, seed):
    """The oracle's ``drop`` of the row as the kernels draw it with `seed` (read back through tc_dropout_mask; the
    probabilities' at the row's heads and token count)."""
    return R.radar_dropout_masks(row['dropout'], seed, row['radar_num_heads'], row['num_query'], layers=row['num_fusion_layers'],
                                 tokens=row['radar_num_tokens'])


MAX_TIED = 6             # influential query-side ReLU ties a training frame may have set apart


def oracle_training(row, drop=None, seed=None, flip=(), tau=None, tied=None):
    """One training iteration of the oracle on the row's frame (frozen decoder: its trace): the trainable weights as
    autograd leaves, head_forward with the masks `drop`, O.loss at the row's class count, backward.
    seed: the frame's (None: the stored one).

    ReLU ties.  Two fp32 evaluation orders of a LayerNorm or a 256-term product part by radar_heads_rig.TIE_TAU, so a ReLU
    input that close to zero may be taken on either side.  On the token side (the radar encoders: thousands of inputs,
    each moving one token's share) they are flipped all at once, `tau`, as radar_heads_rig.tie_sensitivity does.  On the
    query side (a fusion layer's FFN hidden units [Q, 1, 512] and its cls / reg branches [1, Q, 256]) one input moves a
    whole query's contribution to a weight row (test_gpu_radar_input._tied_inputs) -- on a query without a hit it does
    not even depend on the frame -- so these are listed, `tied` (a list that receives (call, query, unit) of every such
    input within TIE_TAU of zero), and taken on the other side one by one, `flip`.
    -> (losses {name: float}, {name: gradient or None} of the trainable parameters)"""
    sd = O.to_torch_sd(R.state_dict(**variant(row)))
    for k, v in sd.items():
        if R.trainable(k):
            v.requires_grad_(True)
    kept = frame_rows(row, 0, frame_seed(row)[0] if seed is None else seed)[1]
    boxes, labels = ground_truth(row)
    Q, plain, calls = row['num_query'], O.F.relu, []

    def relu(x, *args, **kw):
        if not x.requires_grad:
            return plain(x, *args, **kw)
        keep = x.detach() > 0
        if tuple(x.shape) in ((Q, 1, 512), (1, Q, 256)):
            call = len(calls)
            calls.append(1)
            if tied is not None:
                q, u = torch.where((x.detach().abs() < RR.TIE_TAU).reshape(Q, -1))
                tied.extend((call, a, b) for a, b in zip(q.tolist(), u.tolist()))
            for c, q, u in flip:
                if c == call:
                    keep.view(Q, -1)[q, u] ^= True
        elif tau is not None:
            keep = keep ^ (x.detach().abs() < tau)
        return x * keep.to(x.dtype)
    O.F.relu = relu
    try:
        with torch.enable_grad():
            outs = head_forward(row, 0, kept, sd=sd, drop=drop)
            res, _ = O.loss(outs, torch.from_numpy(boxes), torch.from_numpy(labels), sd['code_weights'], num_classes=row['num_classes'])
            sum(res.values()).backward()
    finally:
        O.F.relu = plain
    assert len(calls) == 5 * row['num_fusion_layers'], len(calls)       # FFN, two of the cls and two of the reg branch
    return {k: float(v.detach()) for k, v in res.items()}, {k: v.grad for k, v in sd.items() if R.trainable(k)}


def influential_ties(row, drop=None, seed=None):
    """How far the frame's gradients move when the ReLU inputs nearest to zero are taken on the other side, in
    radar_heads_rig.g8_figures' unit.  All at once, as radar_heads_rig.tie_sensitivity: below half of TIE_BOUND the frame's
    gradients are held to the plain oracle, -> ([], that figure).  Otherwise the query-side ties that move the figures most
    on their own are set apart, as few as bring the figure of all the others at once below half of TIE_BOUND (the other
    half is for another CPU's rounding: which inputs lie within TIE_TAU is decided in fp32) -- the gradient check takes
    each of them on either side, as test_gpu_radar_input does with its two: -> (those ties, the others' figure).
    A frame serves if the figure is below TIE_BOUND with at most MAX_TIED ties set apart."""
    tied = []
    ref = R.GradStats(oracle_training(row, drop, seed, tied=tied)[1])

    def moved(flip, tau=None):
        return float(RR.g8_figures(oracle_training(row, drop, seed, flip=flip, tau=tau)[1], ref))
    rest = moved(tied, RR.TIE_TAU)
    if rest < RR.TIE_BOUND / 2:
        return [], rest
    order = sorted(tied, key=lambda t: -moved([t]))
    for n in range(1, MAX_TIED + 1):
        rest = moved(order[n:], RR.TIE_TAU)
        if rest < RR.TIE_BOUND / 2:
            break
    return order[:n], rest


def matching_oracle(row, grads, drop=None):
    """The oracle's iteration the gradients `grads` are held to: each tie influential_ties sets apart may be taken on
    either side, so they are taken, one after the other, on the side on which g8_figures puts `grads` closer -- a search
    among oracles each of which is a legitimate reference; the caller holds every loss and every gradient to the ONE it
    ends at.  The GPU test comes here only where the plain oracle does not hold the gradients.
    -> (the ties flipped, losses, gradients, the other ties' figure, the ties set apart)"""
    apart, rest = influential_ties(row, drop)

    def figure(res):
        return RR.g8_figures(grads, R.GradStats({k: g for k, g in res[1].items() if grads.get(k) is not None}))
    flip, best = [], oracle_training(row, drop)
    for t in apart:
        other = oracle_training(row, drop, flip=flip + [t])
        if figure(other) < figure(best):
            flip, best = flip + [t], other
    return flip, best[0], best[1], rest, apart
