"""The DETR3D decoder levels' own class scores and boxes (HEAD:277-298) composed from the CPU oracle's pieces: what
``Detr3DHead(outputs='camera')`` returns and tc_decoder_outputs_fwd computes.  A plain helper module (oracle/ is not
edited): for level l

    ref    = inverse_sigmoid(init_reference if l == 0 else inter_references[l - 1])
    cls[l] = cls_branches[l](hs[l])
    t      = reg_branches[l](hs[l])
    t[0:2] = sigmoid(t[0:2] + ref[0:2]);  t[4] = sigmoid(t[4] + ref[2]);  t[0], t[1], t[4] scaled to pc_range (x, y, z)

in the dtype of the state dict (``.double()`` weights and inputs give the fp64 value)."""
import torch

from oracle import transcar_oracle as O
from transcar_amd import configs, synth

PCR = configs.point_cloud_range
BOX_TOL = 5e-5          # metres: fp32 spacing at 50 m is 3.8e-6, the reference and the oracle order add / sigmoid / scale differently


def decoder_outputs(sd, hs, init_ref, inter_refs, pc_range=PCR):
    """hs [L,B,Q,C], init_ref [B,Q,3], inter_refs [L,B,Q,3] -> (cls [L,B,Q,num_classes], box [L,B,Q,code_size])."""
    cls, box = [], []
    for l in range(hs.shape[0]):
        ref = O.inverse_sigmoid(init_ref if l == 0 else inter_refs[l - 1])
        cls.append(O.cls_branch(sd, 'cls_branches.%d' % l, hs[l]))
        t = O.reg_branch(sd, 'reg_branches.%d' % l, hs[l]).clone()
        t[..., 0:2] = (t[..., 0:2] + ref[..., 0:2]).sigmoid()
        t[..., 4:5] = (t[..., 4:5] + ref[..., 2:3]).sigmoid()
        t[..., 0:1] = t[..., 0:1] * (pc_range[3] - pc_range[0]) + pc_range[0]
        t[..., 1:2] = t[..., 1:2] * (pc_range[4] - pc_range[1]) + pc_range[1]
        t[..., 4:5] = t[..., 4:5] * (pc_range[5] - pc_range[2]) + pc_range[2]
        box.append(t)
    return torch.stack(cls), torch.stack(box)


def denormalised_refs(refs, pc_range=PCR):
    """[..., 3] reference points in (0, 1) -> metres (x, y, z)"""
    lo = refs.new_tensor(pc_range[:3])
    hi = refs.new_tensor(pc_range[3:])
    return refs * (hi - lo) + lo


_TRACE = {}


def oracle_trace(with_box_refine, smooth=(4, 6)):
    """The oracle's decoder on the g5_head_tiny rig (feature maps seed 1, state dict seed 3), once per variant:
    -> (sd, hs [L,B,Q,C], init_ref [B,Q,3], inter_refs [L,B,Q,3])."""
    if with_box_refine not in _TRACE:
        kw = {} if with_box_refine else {'with_box_refine': False}
        sd = O.to_torch_sd(synth.make_state_dict(seed=3, **kw))
        feats = synth.make_feats('tiny', seed=1, smooth=smooth)
        l2i = torch.from_numpy(synth.make_lidar2img()).float()[None]
        with torch.no_grad():
            hs, init_ref, inter_refs, _ = O.transformer(sd, [torch.from_numpy(f) for f in feats], PCR, l2i,
                                                        configs.IMG_SHAPE[:2], with_box_refine=with_box_refine)
        _TRACE[with_box_refine] = (sd, hs.permute(0, 2, 1, 3).contiguous(), init_ref, inter_refs)
    return _TRACE[with_box_refine]


_OUT = {}


def oracle_outputs(with_box_refine):
    """decoder_outputs on oracle_trace(with_box_refine), computed once and shared: (cls, box) as numpy arrays"""
    if with_box_refine not in _OUT:
        sd, hs, init_ref, inter_refs = oracle_trace(with_box_refine)
        with torch.no_grad():
            cls, box = decoder_outputs(sd, hs, init_ref, inter_refs)
        _OUT[with_box_refine] = (cls.numpy(), box.numpy())
    return _OUT[with_box_refine]
