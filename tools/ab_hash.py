import hashlib, sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch, bench
from transcar_amd import detr3d_head as D
dev = torch.device('cuda:0')
torch.set_grad_enabled(False)
head, _ = bench.build_head(dev)
# every kernel variant of the row chains: 32, 16 f16x2, 16 f32, 8, 4 rows
for rows, mp in ((32, None), (16, None), (16, 'f32'), (8, None), (4, None)):
    for B in (9, 2):
        inp = bench.make_inputs(head, dev, 'res101', B, seed=3, host_feats=False)
        o = head.forward_nhwc(inp['nhwc'], inp['l2i'], inp['hw'], inp['tokens'], inp['pad_mult'],
                              options=D.head_options(tile_rows=rows, matrix_path=mp))
        h = hashlib.sha256()
        for k in ('all_cls_scores', 'all_bbox_preds'):
            h.update(o[k].contiguous().cpu().numpy().tobytes())
        print('rows', rows, mp or '', 'B', B, h.hexdigest()[:16], flush=True)
# one FusionTrainer iteration in its deterministic mode, twice each: one frame runs the 4-row training chains, two frames
# (1800 rows) the 8-row ones.  The loss values meet in float atomics of the loss kernel and are not reproducible bit for
# bit: their sum is printed with every digit, to be held against the other build's own run-to-run spread
for B in (1, 2):
    inp = bench.make_inputs(head, dev, 'res101', B, seed=3, host_feats=False)
    for run in (0, 1, 2):
        thead, tr, gts, lbs = bench._train_setup(head, dev, 0, B, 1, deterministic=True)
        with torch.enable_grad():
            losses = tr.step_fused_nhwc(inp['nhwc'], inp['l2i'], inp['hw'], inp['tokens'], inp['pad_mult'], gts, lbs, update=False)
        torch.cuda.synchronize()
        g = hashlib.sha256(tr.bucket.grads.contiguous().cpu().numpy().tobytes()).hexdigest()[:16]
        vals = [float(losses[k]) for k in sorted(losses)]
        print('rows train B', B, 'run', run, 'grads', g, 'loss sum %.17g' % sum(vals), 'largest term %.17g' % max(vals), flush=True)
