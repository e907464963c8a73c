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
# the other ways into the native host layer, two frames each (8-row chains unless a case says otherwise): every line starts
# with 'rows' (tools/ab_bench.sh keeps those)
import ctypes as C
from transcar_amd import _lib as L, ops


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().cpu().numpy().tobytes())
    return h.hexdigest()[:16]


B = 2
inp = bench.make_inputs(head, dev, 'res101', B, seed=3, host_feats=False)
fwd = lambda **kw: head.forward_nhwc(inp['nhwc'], inp['l2i'], inp['hw'], inp['tokens'], inp['pad_mult'], **kw)
outs = lambda o: digest(o['all_cls_scores'], o['all_bbox_preds'])
whole = fwd(aux=True)
aux = whole['aux']
print('rows forward aux B', B, outs(whole), digest(*[aux[k] for k in sorted(aux)]), flush=True)
print('rows forward two-phase B', B, outs(fwd(fill_tokens=lambda: None)), flush=True)
print('rows forward decoder-dropout B', B, outs(fwd(options=D.head_options(decoder_dropout_p=0.1, dropout_seed=7))), flush=True)
print('rows forward hits-first B', B, outs(fwd(options=D.head_options(radar_compact=True))), flush=True)
print('rows forward unfused B', B, outs(fwd(options=D.head_options(unfused=True))), flush=True)
print('rows forward pre-gather 16 B', B, outs(fwd(options=D.head_options(tile_rows=16, cam_pregather=True))), flush=True)
# tc_radar_fusion_fwd: all layers from the decoder's outputs, then layers 1 .. on the K | V the first call left in `ws`
hs_last, ref_last = aux['inter_states'][-1].contiguous(), aux['inter_references'][-1].contiguous()
ws = torch.empty(L.lib().tc_head_workspace_bytes(C.byref(head._packed_view), B, inp['tokens'].shape[1]), dtype=torch.uint8, device=dev)
cls, box, hits = ops.radar_fusion(head, hs_last, ref_last, aux['last_box'], inp['tokens'], inp['pad_mult'], ws=ws)
print('rows fusion first 0 B', B, digest(cls, box, hits), flush=True)
if head.num_fusion_layers > 1:
    reuse = D.head_options()
    reuse.reuse_radar_kv = 1
    part = ops.radar_fusion(head, hs_last, ref_last, box[0].contiguous(), inp['tokens'], inp['pad_mult'], first_layer=1, options=reuse, ws=ws)
    print('rows fusion first 1 reuse B', B, digest(*[t[1:] for t in part]), flush=True)
# one decoder layer's chain alone (layer 1 on layer 0's outputs; its attention output is a stand-in: layer 0's state)
pv = head._packed_view
x0, r0 = aux['inter_states'][0].contiguous(), aux['inter_references'][0].contiguous()
tail = ops.decoder_layer_tail(pv.layers[1], pv.layers[2].self_attn.in_proj, inp['nhwc'], x0, x0, head.query_embedding.weight,
                              inp['l2i'], r0, head.pc_range, inp['hw'], code_size=head.code_size)
print('rows decoder_layer_tail B', B, digest(*tail), flush=True)
# the two training forwards of the radar stack on one frame, dropout on with a fixed seed: outputs and the whole tape
w = head.head_weights()
head.sync_packed_weights()
T1 = inp['tokens'].shape[1]
one = [t[:1].contiguous() for t in (hs_last, ref_last, aux['last_box'], inp['tokens'])]
for name, fn, weights in (('tc_radar_train_fwd_fused', L.lib().tc_radar_train_fwd_fused, head._packed_view),
                          ('tc_radar_train_fwd', L.lib().tc_radar_train_fwd, w)):
    tape = L.device_bytes(dev, L.lib().tc_radar_train_tape_bytes, C.byref(w), 1, T1)
    tape.zero_()
    t_cls = torch.zeros((head.num_fusion_layers, 1, head.num_query, head.cls_out_channels), dtype=torch.float32, device=dev)
    t_box = torch.zeros((head.num_fusion_layers, 1, head.num_query, head.code_size), dtype=torch.float32, device=dev)
    L.check(fn(C.byref(weights), one[0].data_ptr(), one[1].data_ptr(), one[2].data_ptr(), one[3].data_ptr(), 1, T1,
               int(inp['pad_mult']), t_cls.data_ptr(), t_box.data_ptr(), tape.data_ptr(), tape.numel(), 0.1, 5, L.stream_ptr()), name)
    torch.cuda.synchronize()
    print('rows', name, 'B 1', digest(t_cls, t_box), 'tape', digest(tape), flush=True)
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
