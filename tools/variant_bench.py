#!/usr/bin/env python3
"""What one keyword of the head's configuration costs: frames/s of the bench's res101 head (seeded weights,
configs.head_cfg() with that keyword overridden) through the same FramePipeline measurement as bench.py's headline
(bench._pipeline_rate: its lanes, the resident frames per launch, whole launches per window), interleaved over the
values.  The first value is the base of `relative_to_first`.
    python tools/variant_bench.py --vary num_points 1 5 [--rounds 3] [--steps 20]        (one JSON line)
    python tools/variant_bench.py --vary num_levels 4 3 2 1
    python tools/variant_bench.py --vary num_heads 8 4 16
    python tools/variant_bench.py --vary radar_num_heads 8 4 16
    python tools/variant_bench.py --vary with_box_refine 1 0
    python tools/variant_bench.py --vary feedforward_channels 512 256 1024 2048
    python tools/variant_bench.py --vary radar_num_tokens 1500 4096 --radar-points 255 3000
    python tools/variant_bench.py --vary radar_in_dims 36 4 --radar-num-tokens 4096 --radar-points 3000

num_points       Detr3DCrossAtten.num_points (DESIGN.md "num_points").
num_levels       the head is fed the FIRST L res101 levels; L = 4 is the headline configuration, L < 4 runs the generic
                 chain kernels (DESIGN.md "num_levels < 4").
num_heads        the decoder self-attention's head count: 8 is the headline (head dimension 32); 4 and 16 run the
                 attention cores' D = 64 and D = 16 instantiations.  The state dict does not depend on it.
radar_num_heads  the radar fusion attention's head count (8 is the headline): the same kernels with 16 / 8 / 4 lanes per
                 head.  The state dict does not depend on it either.
radar_num_tokens the head's token count N (1500 is the headline) with --radar-points radar points per frame (one count per
                 value, or one for all; default the bench's 255): the frames are the bench's, with that many points.  The
                 state dict does not depend on N.  Also reported: `radar_chain_us`, the fusion chain alone over one launch's
                 frames (tc_radar_fusion_fwd on encoded tokens; with the three fills of its output tensors).
radar_in_dims    features per token (36 is the headline) at --radar-num-tokens N: the rows are the first F of the 36 columns.
                 The fusion chain reads a token's x, y at a stride of 4 F bytes: its time against F = 4 is what the stride costs.
feedforward_channels  the decoder layers' FFN width (512 is the headline; DESIGN.md "feedforward_channels"): the decoder chains
                 run ceil(F / 512) chunks of the FFN's two steps.  The fusion layers' FFN stays 512 wide.
with_box_refine  both heads carry synth.make_state_dict(with_box_refine=False)'s shared branches; the results are keyed
                 'refine' / 'norefine' and `norefine_over_refine` is reported, as profiles/box_refine_bench.json has it."""
import argparse
import ctypes
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import transcar_amd as T  # noqa: E402
from transcar_amd import configs, synth  # noqa: E402

KEYWORDS = ('num_points', 'num_levels', 'num_heads', 'radar_num_heads', 'with_box_refine', 'radar_num_tokens', 'radar_in_dims',
            'feedforward_channels')


def build_head(dev, keyword, value, **cfg_kw):
    sd_kw = {'num_heads': {}, 'radar_num_heads': {}, 'radar_num_tokens': {}, 'radar_in_dims': dict(radar_in=value),
             'with_box_refine': dict(with_box_refine=False)}.get(keyword, {keyword: value})
    head = T.build_head(configs.head_cfg(**dict(cfg_kw, **{keyword: bool(value) if keyword == 'with_box_refine' else value})))
    head.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(seed=3, **sd_kw).items()}, strict=True)
    return head.to(dev).eval()


def shapes_of(keyword, value):
    """a LEVEL_SHAPES key: res101, or its first num_levels levels (bench.make_inputs looks the shapes up by name)"""
    if keyword != 'num_levels' or value == 4:
        return 'res101'
    key = 'res101_first%d' % value
    configs.LEVEL_SHAPES[key] = configs.LEVEL_SHAPES['res101'][:value]
    return key


def radar_lane(head, dev, fpl, seed, points, tokens_T=None):
    """bench.make_inputs' lane with `points` radar points per frame packed for the head's token count and feature count"""
    from transcar_amd import radar as R
    inp = bench.make_inputs(head36(head, dev), dev, 'res101', fpl, seed=seed, host_feats=False)
    o = head36(head, dev).forward_nhwc(inp['nhwc'], inp['l2i'], inp['hw'], inp['tokens'], inp['pad_mult'], aux=True)
    r = o['aux']['inter_references'][-1].cpu().numpy().astype(np.float64)
    pcr, rows = configs.point_cloud_range, []
    for b in range(fpl):
        c = np.round(np.stack([r[b, :, 0] * (pcr[3] - pcr[0]) + pcr[0], r[b, :, 1] * (pcr[4] - pcr[1]) + pcr[1]], 1), 2)
        f36 = R.build_radar_features(synth.make_radar_frame(seed=2 + b, n_per_radar=points // 5, centres=c))
        rows.append(f36[:, :head.radar_in_dims])
    tok, pm = R.pack_tokens(rows, T=tokens_T, num_tokens=head.radar_num_tokens)
    inp.update(tokens=torch.from_numpy(tok).to(dev), pad_mult=pm, radar_feats=rows)
    return inp


_HEAD36 = {}


def head36(head, dev):
    """the headline head, for the radar-free pass that says where a lane's frames put their radar points (the decoder reads no
    radar: every radar variant shares it)"""
    if head.radar_in_dims == 36 and head.radar_num_tokens == 1500:
        return head
    if 'h' not in _HEAD36:
        _HEAD36['h'] = build_head(dev, 'radar_num_tokens', 1500)
    return _HEAD36['h']


def radar_rate(head, dev, args, fpl, points, tokens_T=None):
    """bench._pipeline_rate on radar_lane's lanes -> (frames/s, radar chain us per launch of fpl frames, T)"""
    from transcar_amd import ops
    from transcar_amd.detr3d_head import head_options
    from transcar_amd.pipeline import FramePipeline
    lanes = [radar_lane(head, dev, fpl, 41 + 5 * i, points, tokens_T) for i in range(max(1, args.lanes))]
    pipe = FramePipeline(head, lanes)
    for _ in range(3):
        for _ in range(fpl * pipe.lanes):
            pipe.submit()
        pipe.flush()
        torch.cuda.synchronize()

    def sync():
        pipe.flush()
        torch.cuda.synchronize()
    rounds = max(2, -(-max(20, args.steps) // (fpl * pipe.lanes)))
    rate = 1.0 / bench._replay_rate(pipe.submit, sync, rounds * fpl * pipe.lanes, min_s=0.6)
    inp = lanes[0]
    o = head.forward_nhwc(inp['nhwc'], inp['l2i'], inp['hw'], inp['tokens'], inp['pad_mult'], aux=True)
    aux = o['aux']
    hs, ref, box = aux['inter_states'][-1].contiguous(), aux['inter_references'][-1].contiguous(), aux['last_box']
    ws = T._lib.device_bytes(dev, T.lib().tc_head_workspace_bytes, ctypes.byref(head._packed_view), fpl, inp['tokens'].shape[1])
    ops.radar_fusion(head, hs, ref, box, inp['tokens'], inp['pad_mult'], ws=ws)        # (encodes the tokens into ws)
    opt = head_options(tile_rows=pipe.tile_rows_of())
    opt.reuse_radar_kv = 1
    chain_ms = bench.time_events(lambda: ops.radar_fusion(head, hs, ref, box, inp['tokens'], inp['pad_mult'], options=opt, ws=ws),
                                 iters=20)
    T_tok = int(inp['tokens'].shape[1])
    del pipe, lanes
    torch.cuda.synchronize()
    return rate, chain_ms * 1e3, T_tok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--vary', nargs='+', required=True, metavar=('KEYWORD', 'VALUE'))
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--lanes', type=int, default=3)
    ap.add_argument('--radar-points', type=int, nargs='+', default=[255], help='radar points per frame (radar_* keywords)')
    ap.add_argument('--radar-T', type=int, default=None, help='materialised tokens T (default: the smallest that holds the frames)')
    ap.add_argument('--radar-num-tokens', type=int, default=1500, help='the token count beside --vary radar_in_dims')
    a = ap.parse_args()
    keyword, values = a.vary[0], [int(v) for v in a.vary[1:]]
    if keyword not in KEYWORDS or not values:
        ap.error('--vary takes one of %s and at least one value' % ', '.join(KEYWORDS))
    refine = keyword == 'with_box_refine'
    label = {v: (('norefine', 'refine')[bool(v)] if refine else str(v)) for v in values}
    torch.set_grad_enabled(False)
    dev = torch.device('cuda:0')
    radar = keyword in ('radar_num_tokens', 'radar_in_dims')
    if radar and len(a.radar_points) not in (1, len(values)):
        ap.error('--radar-points takes one count, or one per value')
    points = dict(zip(values, a.radar_points * len(values) if len(a.radar_points) == 1 else a.radar_points))
    cfg_kw = dict(radar_num_tokens=a.radar_num_tokens) if keyword == 'radar_in_dims' else {}
    heads = {v: build_head(dev, keyword, v, **cfg_kw) for v in values}
    fpl = bench.auto_frames_per_launch(heads[values[0]], dev)
    args = types.SimpleNamespace(lanes=a.lanes, warmup_s=0.5, steps=a.steps)
    rates = {v: [] for v in values}
    chain_us, tokens_T = {v: [] for v in values}, {}
    for _ in range(a.rounds):
        for v in values:
            if radar:
                r, us, tokens_T[label[v]] = radar_rate(heads[v], dev, args, fpl, points[v], a.radar_T)
                chain_us[v].append(us)
                rates[v].append(r)
                continue
            r, pipe, lanes = bench._pipeline_rate(heads[v], dev, args, shapes_of(keyword, v), fpl, None)
            rates[v].append(r)
            del pipe, lanes
            torch.cuda.synchronize()
    res = {'metric': 'frames_per_s', 'vary': keyword,
           'shapes': 'res101, first L levels' if keyword == 'num_levels' else 'res101', 'frames_per_launch': fpl,
           'lanes': a.lanes, 'rounds': a.rounds, 'rates': {label[v]: rates[v] for v in values},
           'median': {label[v]: float(np.median(rates[v])) for v in values}}
    if radar:
        res.update(radar_points={label[v]: points[v] for v in values}, tokens_T=tokens_T,
                   radar_num_tokens={label[v]: heads[v].radar_num_tokens for v in values},
                   radar_chain_us={label[v]: float(np.median(chain_us[v])) for v in values})
    base = res['median'][label[values[0]]]
    res['relative_to_first'] = {label[v]: res['median'][label[v]] / base for v in values}
    if refine and set(label.values()) == {'refine', 'norefine'}:
        res['norefine_over_refine'] = res['median']['norefine'] / res['median']['refine']
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
