"""Tensor-level wrappers over the C ABI (torch is only plumbing here: device
memory, the current HIP stream).  Every function requires fp32 tensors on a
HIP device and raises if the library is missing -- there is no CPU path.

Each wrapper names the reference operator it replaces; see
include/transcar_hip.h for the exact contracts.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib as L


def _p(t):
    if t is None:
        return None
    return C.c_void_p(t.data_ptr())


def _chk(t, name):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32
            and t.is_contiguous()):
        raise L.TransCARHipError(
            '%s must be a contiguous fp32 tensor on the GPU (got %s)' % (
                name, (t.dtype, t.device, t.is_contiguous())
                if torch.is_tensor(t) else type(t)))
    return t


def linear_view(weight, bias):
    return L.tc_linear(_p(weight), _p(bias))


def lnorm_view(weight, bias):
    return L.tc_lnorm(_p(weight), _p(bias))


# --------------------------------------------------------------------------
# layout
# --------------------------------------------------------------------------
def to_nhwc(feat, out=None):
    """[B,N,C,H,W] (or [BN,C,H,W]) NCHW fp32 -> [B*N,H,W,C] contiguous.

    A tensor that is already channels-last in memory (the FPN ran in
    ``torch.channels_last``) is reinterpreted without a copy."""
    if feat.dim() == 5:
        feat = feat.reshape(-1, *feat.shape[2:])
    n, c, h, w = feat.shape
    if feat.is_contiguous(memory_format=torch.channels_last) and \
            not feat.is_contiguous():
        return feat.permute(0, 2, 3, 1)           # zero-copy NHWC view
    _chk(feat, 'feat')
    if out is None:
        out = torch.empty((n, h, w, c), dtype=torch.float32,
                          device=feat.device)
    L.check(L.lib().tc_nchw_to_nhwc(_p(feat), _p(out), n, c, h, w, L.stream_ptr()),
            'tc_nchw_to_nhwc')
    return out


def to_nhwc_levels(feats, out=None):
    """All FPN levels of a frame, NCHW -> NHWC, in ONE launch
    (tc_nchw_to_nhwc_levels).  feats: list of [B,N,C,H,W] / [BN,C,H,W] fp32;
    out: optional list of preallocated [BN,H,W,C] tensors (a lane's static
    inputs).  Levels that are already channels-last in memory are taken
    zero-copy and left out of the launch."""
    res, todo = [], []
    for l, f in enumerate(feats):
        if f.dim() == 5:
            f = f.reshape(-1, *f.shape[2:])
        if f.is_contiguous(memory_format=torch.channels_last) and not f.is_contiguous() \
                and out is None:
            res.append(f.permute(0, 2, 3, 1))
            continue
        _chk(f, 'feats[%d]' % l)
        n, c, h, w = f.shape
        o = out[l] if out is not None else torch.empty((n, h, w, c), dtype=torch.float32,
                                                       device=f.device)
        if out is not None and (tuple(o.shape) != (n, h, w, c) or not o.is_contiguous()):
            raise L.TransCARHipError('out[%d] must be a contiguous [%d,%d,%d,%d] tensor' % (l, n, h, w, c))
        res.append(o)
        todo.append((f, o))
    if todo:
        k = len(todo)
        if len({(f.shape[0], f.shape[1]) for f, _ in todo}) != 1:
            raise L.TransCARHipError('all levels must have the same image count and channels')
        src = (C.c_void_p * k)(*[f.data_ptr() for f, _ in todo])
        dst = (C.c_void_p * k)(*[o.data_ptr() for _, o in todo])
        hs = (C.c_int * k)(*[f.shape[2] for f, _ in todo])
        ws = (C.c_int * k)(*[f.shape[3] for f, _ in todo])
        L.check(L.lib().tc_nchw_to_nhwc_levels(src, dst, k, todo[0][0].shape[0],
                                               todo[0][0].shape[1], hs, ws, L.stream_ptr()),
                'tc_nchw_to_nhwc_levels')
    return res


def feats_view(feats_nhwc):
    """list of [B*N,H,W,C] -> tc_feats_nhwc."""
    fv = L.tc_feats_nhwc()
    if not 1 <= len(feats_nhwc) <= L.TC_MAX_LEVELS:
        raise L.TransCARHipError('%d feature levels (1 .. %d supported)'
                                 % (len(feats_nhwc), L.TC_MAX_LEVELS))
    fv.num_levels = len(feats_nhwc)
    for i, f in enumerate(feats_nhwc):
        if not (f.is_cuda and f.dtype == torch.float32 and f.is_contiguous()):
            raise L.TransCARHipError('NHWC level %d must be contiguous fp32 '
                                     'on the GPU' % i)
        fv.data[i] = f.data_ptr()
        fv.H[i] = f.shape[1]
        fv.W[i] = f.shape[2]
    return fv


# --------------------------------------------------------------------------
# operators
# --------------------------------------------------------------------------
def linear(x, weight, bias, x2=None, res=None, act=0):
    """nn.Linear (+ optional x2 added to the input, residual, ReLU)."""
    _chk(x, 'x'); _chk(weight, 'weight')
    M = x.numel() // x.shape[-1]
    K, N = x.shape[-1], weight.shape[0]
    y = torch.empty(x.shape[:-1] + (N,), dtype=torch.float32, device=x.device)
    L.check(L.lib().tc_linear_fwd(_p(x), _p(x2), _p(weight), _p(bias), _p(res),
                                  _p(y), M, K, N, act, L.stream_ptr()),
            'tc_linear_fwd')
    return y


def add_layernorm(a, b, gamma, beta, relu=False):
    """LayerNorm(a (+ b)), eps 1e-5, optional ReLU."""
    _chk(a, 'a')
    Cdim = a.shape[-1]
    y = torch.empty_like(a)
    L.check(L.lib().tc_add_layernorm_fwd(_p(a), _p(b), _p(gamma), _p(beta),
                                         _p(y), a.numel() // Cdim, Cdim,
                                         1 if relu else 0, L.stream_ptr()),
            'tc_add_layernorm_fwd')
    return y


def refine_reference(reg_out, ref):
    """XFMR:195-203: sigmoid(reg_out[..., {0,1,4}] + inverse_sigmoid(ref))."""
    _chk(reg_out, 'reg_out'); _chk(ref, 'ref')
    new_ref = torch.empty_like(ref)
    L.check(L.lib().tc_refine_reference_fwd(
        _p(reg_out), reg_out.shape[-1], _p(ref), _p(new_ref),
        ref.numel() // 3, L.stream_ptr()), 'tc_refine_reference_fwd')
    return new_ref


def cam_sample_fuse(feats_nhwc, lidar2img, ref, attn_logits, pc_range, img_hw,
                    num_cams=6, return_mask=False, num_points=1):
    """feature_sampling + sigmoid-weighted (cam, level) reduction
    (XFMR:365-373, 381-422).  ref [B,Q,3], attn_logits [B,Q,N*P*L] -> [B,Q,C];
    with num_points P > 1 level value (n, l) weighs sum_p sigmoid(logit[n,p,l])."""
    _chk(ref, 'ref'); _chk(attn_logits, 'attn_logits'); _chk(lidar2img, 'l2i')
    B, Q = ref.shape[:2]
    Cdim = feats_nhwc[0].shape[-1]
    fv = feats_view(feats_nhwc)
    L.check_num_points(num_points, num_cams, fv.num_levels)
    out = torch.empty((B, Q, Cdim), dtype=torch.float32, device=ref.device)
    vis = torch.empty((B, Q, num_cams), dtype=torch.uint8,
                      device=ref.device) if return_mask else None
    if num_points == 1:
        L.check(L.lib().tc_cam_sample_fuse_fwd(
            C.byref(fv), B, Q, Cdim, num_cams, _p(lidar2img), _p(ref),
            _p(attn_logits), L.f6(pc_range), float(img_hw[0]), float(img_hw[1]),
            _p(out), _p(vis), None, L.stream_ptr()), 'tc_cam_sample_fuse_fwd')
    else:
        L.check(L.lib().tc_cam_sample_fuse_points_fwd(
            C.byref(fv), B, Q, Cdim, num_cams, int(num_points), _p(lidar2img),
            _p(ref), _p(attn_logits), L.f6(pc_range), float(img_hw[0]),
            float(img_hw[1]), _p(out), _p(vis), None, L.stream_ptr()),
            'tc_cam_sample_fuse_points_fwd')
    return (out, vis) if return_mask else out


def cross_atten(aw, oproj, pe, feats_nhwc, query, query_pos, lidar2img, ref,
                pc_range, img_hw, num_cams=6, num_points=1):
    """Detr3DCrossAtten.forward (XFMR:302-378); query/query_pos [B,Q,C];
    aw = attention_weights [num_cams*num_points*L, C]."""
    _chk(query, 'query'); _chk(query_pos, 'query_pos'); _chk(ref, 'ref')
    B, Q, Cdim = query.shape
    fv = feats_view(feats_nhwc)
    L.check_num_points(num_points, num_cams, fv.num_levels)
    out = torch.empty_like(query)
    if num_points == 1:
        nbytes = L.lib().tc_cross_atten_workspace_bytes(B, Q, Cdim, num_cams,
                                                        fv.num_levels)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=query.device)
        L.check(L.lib().tc_cross_atten_fwd(
            C.byref(aw), C.byref(oproj), C.byref(pe), C.byref(fv), B, Q, Cdim,
            num_cams, _p(query), _p(query_pos), _p(lidar2img), _p(ref),
            L.f6(pc_range), float(img_hw[0]), float(img_hw[1]), _p(out), _p(ws),
            nbytes, L.stream_ptr()), 'tc_cross_atten_fwd')
        return out
    nbytes = L.lib().tc_cross_atten_points_workspace_bytes(
        B, Q, Cdim, num_cams, fv.num_levels, int(num_points))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=query.device)
    L.check(L.lib().tc_cross_atten_points_fwd(
        C.byref(aw), C.byref(oproj), C.byref(pe), C.byref(fv), B, Q, Cdim,
        num_cams, int(num_points), _p(query), _p(query_pos), _p(lidar2img),
        _p(ref), L.f6(pc_range), float(img_hw[0]), float(img_hw[1]), _p(out),
        _p(ws), nbytes, L.stream_ptr()), 'tc_cross_atten_points_fwd')
    return out


def self_attn(mha, x, pos, num_heads=8):
    """mmcv MultiheadAttention wrapper: x + out_proj(MHA(x+pos, x+pos, x))."""
    _chk(x, 'x'); _chk(pos, 'pos')
    B, Q, Cdim = x.shape
    nbytes = L.lib().tc_self_attn_workspace_bytes(B, Q, Cdim)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    out = torch.empty_like(x)
    L.check(L.lib().tc_self_attn_fwd(C.byref(mha), _p(x), _p(pos), _p(out), B,
                                     Q, Cdim, num_heads, _p(ws), nbytes,
                                     L.stream_ptr()), 'tc_self_attn_fwd')
    return out


def sdpa(q, k, vt, num_heads=8, matrix_path='f32', head_dim=None):
    """The self-attention core on projected operands (tc_sdpa_fwd; matrix_path='f16x2': tc_sdpa_fwd_f16x2, the
    same on the f16 matrix cores with two-plane operands):
    q, k [B,Q,C] token-major (q pre-scaled by log2(e)/sqrt(head_dim)),
    vt [B,C,qpad] = V transposed, qpad = round_up(Q,16) -> [B,Q,C].
    head_dim=None: the entry points above (head dimension 32); 16, 32 or 64: tc_sdpa_fwd_hd /
    tc_sdpa_fwd_f16x2_hd, C = num_heads * head_dim."""
    B, Q, Cdim = q.shape
    qk = torch.cat((q, k), -1).contiguous()                 # the layout the chains produce
    _chk(qk, 'qk'); _chk(vt, 'vt')
    out = torch.empty((B, Q, Cdim), dtype=torch.float32, device=q.device)
    if head_dim is not None:
        if num_heads * int(head_dim) != Cdim or vt.shape[1] != Cdim:
            raise L.TransCARHipError('sdpa: num_heads=%r * head_dim=%r does not match C=%d'
                                     % (num_heads, head_dim, Cdim))
        if matrix_path == 'f16x2':
            L.check(L.lib().tc_sdpa_fwd_f16x2_hd(qk.data_ptr(), _p(vt), vt.shape[-1], _p(out), Cdim, B, Q, num_heads,
                                                 int(head_dim), L.stream_ptr()), 'tc_sdpa_fwd_f16x2_hd')
        else:
            L.check(L.lib().tc_sdpa_fwd_hd(qk.data_ptr(), qk.data_ptr() + 4 * Cdim, 2 * Cdim, _p(vt), vt.shape[-1],
                                           _p(out), Cdim, B, Q, num_heads, int(head_dim), L.stream_ptr()),
                    'tc_sdpa_fwd_hd')
        return out
    if matrix_path == 'f16x2':
        ws = torch.empty(L.lib().tc_sdpa_f16x2_workspace_bytes(B, Q, num_heads), dtype=torch.uint8, device=q.device)
        L.check(L.lib().tc_sdpa_fwd_f16x2(qk.data_ptr(), _p(vt), vt.shape[-1], _p(out), Cdim, B, Q, num_heads,
                                          ws.data_ptr(), ws.numel(), L.stream_ptr()), 'tc_sdpa_fwd_f16x2')
        return out
    L.check(L.lib().tc_sdpa_fwd(qk.data_ptr(), qk.data_ptr() + 4 * Cdim, 2 * Cdim, _p(vt),
                                vt.shape[-1], _p(out), Cdim, B, Q, num_heads, L.stream_ptr()),
            'tc_sdpa_fwd')
    return out


def decoder_layer_tail(packed_layer, packed_next_in_proj, feats_nhwc, attn_o, x_in,
                       query_embedding, lidar2img, ref_in, pc_range, img_hw, code_size=10,
                       num_cams=6, tile_rows=0, matrix_path=0, ffn_dims=512):
    """One decoder layer after its attention core as the fused row chain
    (tc_decoder_layer_tail_fwd_ffn; ffn_dims: the feedforward_channels of the
    head the packed layer comes from, which the C layer struct does not carry
    either).  Detr3DCrossAtten.num_points = 1 only (the C
    layer struct does not carry num_points; P > 1 heads run through
    tc_head_forward).  packed_*: members of the head's packed view
    (``head._packed_view.layers[l]``, ``.layers[l + 1].self_attn.in_proj`` or
    None).  matrix_path: TC_MATRIX_* of 16-row tiles (tc_head_options.matrix_path).
    Returns (hs [B,Q,C], ref_out [B,Q,3], qk [B,Q,2C], vt [B,C,qpad])."""
    for n, t in (('attn_o', attn_o), ('x_in', x_in), ('ref_in', ref_in), ('lidar2img', lidar2img)):
        _chk(t, n)
    B, Q, Cdim = x_in.shape
    qpad = ((Q + 15) // 16) * 16
    dev = x_in.device
    hs = torch.empty((B, Q, Cdim), dtype=torch.float32, device=dev)
    ref_out = torch.empty((B, Q, 3), dtype=torch.float32, device=dev)
    qk = torch.zeros((B, Q, 2 * Cdim), dtype=torch.float32, device=dev)
    vt = torch.zeros((B, Cdim, qpad), dtype=torch.float32, device=dev)
    fv = feats_view(feats_nhwc)
    L.check(L.lib().tc_decoder_layer_tail_fwd_ffn(
        C.byref(packed_layer), C.byref(packed_next_in_proj) if packed_next_in_proj is not None else None,
        C.byref(fv), B, Q, num_cams, code_size, _p(attn_o), _p(x_in), _p(query_embedding),
        _p(lidar2img), _p(ref_in), L.f6(pc_range), float(img_hw[0]), float(img_hw[1]), _p(hs),
        _p(ref_out), _p(qk), _p(vt), qpad, int(tile_rows) | (int(matrix_path) << 8), int(ffn_dims), L.stream_ptr()),
        'tc_decoder_layer_tail_fwd_ffn')
    return hs, ref_out, qk, vt


def radar_fusion(head, hs_last, ref_last, prev_box, tokens, pad_mult, first_layer=0,
                 num_layers=None, options=None, ws=None):
    """The radar part of the head from given decoder outputs (tc_radar_fusion_fwd):
    encoders + fusion layers [first_layer, first_layer + num_layers); num_layers=None:
    up to the head's last one.  Returns (all_cls [N,B,Q,ncls], all_box [N,B,Q,code],
    hits [N,B,Q]), N = head.num_fusion_layers; only the slices of the layers that ran are
    written (the rest is NaN / -1)."""
    NF = head.num_fusion_layers
    if num_layers is None:
        num_layers = NF - int(first_layer)
    head.head_weights()
    head.sync_packed_weights()
    pv = head._packed_view
    B, Q = hs_last.shape[:2]
    T = tokens.shape[1]
    dev = hs_last.device
    for n, t in (('hs_last', hs_last), ('prev_box', prev_box), ('tokens', tokens)):
        _chk(t, n)
    nbytes = L.lib().tc_head_workspace_bytes(C.byref(pv), B, T)
    if ws is None:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    cls = torch.full((NF, B, Q, head.cls_out_channels), float('nan'), dtype=torch.float32, device=dev)
    box = torch.full((NF, B, Q, head.code_size), float('nan'), dtype=torch.float32, device=dev)
    hits = torch.full((NF, B, Q), -1, dtype=torch.int32, device=dev)
    L.check(L.lib().tc_radar_fusion_fwd(
        C.byref(pv), _p(hs_last), _p(ref_last), _p(prev_box), _p(tokens), B, T, int(pad_mult),
        int(first_layer), int(num_layers), _p(cls), _p(box), _p(hits),
        C.byref(options) if options is not None else None, _p(ws), ws.numel() * ws.element_size(), L.stream_ptr()),
        'tc_radar_fusion_fwd')
    return cls, box, hits


def radar_gated_xattn(mha, query, centre_xy, box, radar_feat, radar_xy,
                      pad_mult, rmin, rmax, num_heads=8):
    """One radar fusion layer's gated attention step (HEAD:549-581).
    Returns (query + attention on hit rows, hit_counts [B,Q])."""
    for n, t in (('query', query), ('centre_xy', centre_xy), ('box', box),
                 ('radar_feat', radar_feat), ('radar_xy', radar_xy)):
        _chk(t, n)
    B, Q, Cdim = query.shape
    T = radar_feat.shape[1]
    nbytes = L.lib().tc_radar_xattn_workspace_bytes(B, Q, T, Cdim)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=query.device)
    out = torch.empty_like(query)
    hits = torch.empty((B, Q), dtype=torch.int32, device=query.device)
    L.check(L.lib().tc_radar_gated_xattn_fwd(
        C.byref(mha), _p(query), _p(centre_xy), _p(box), box.shape[-1],
        _p(radar_feat), _p(radar_xy), B, Q, T, Cdim, num_heads, int(pad_mult),
        float(rmin), float(rmax), _p(out), _p(hits), _p(ws), nbytes,
        L.stream_ptr()), 'tc_radar_gated_xattn_fwd')
    return out, hits


def radar_raw_arrays(frame):
    """Raw radar of one sample (transcar_amd/radar.py layout) -> what tc_radar_build_tokens
    takes: (raw [N,18] float64, times [N] float64, chan_start [6], radar_rot [5,9], lidar_rot [9]),
    all numpy / host.  The only arithmetic here is the quaternion -> rotation matrix conversion."""
    from . import radar as R
    raws, times, start = [], [], [0]
    for chan in R.RADAR_CHANNELS:
        p = np.asarray(frame['points'][chan], dtype=np.float64)          # [18,n]
        t = np.asarray(frame['times'][chan], dtype=np.float64).reshape(-1)
        raws.append(p.T)
        times.append(t)
        start.append(start[-1] + p.shape[1])
    raw = np.ascontiguousarray(np.concatenate(raws, 0)) if start[-1] else np.zeros((0, 18))
    # the six quaternions at once (same formula and operation order as radar.quaternion_rotation_matrix)
    q = np.asarray([frame['radar_rot'][c] for c in R.RADAR_CHANNELS] + [frame['lidar_rot']], dtype=np.float64)
    q = q / np.asarray([np.linalg.norm(v) for v in q])[:, None]     # (the scalar norm of the host builder: bit-identical)
    w_, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    m = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w_), 2 * (x * z + y * w_),
                  2 * (x * y + z * w_), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w_),
                  2 * (x * z - y * w_), 2 * (y * z + x * w_), 1 - 2 * (x * x + y * y)], axis=1)
    rr, lr = m[:-1], m[-1]
    return raw, np.concatenate(times) if start[-1] else np.zeros(0), np.asarray(start, np.int32), rr, lr


def radar_build_tokens(frame, T, device, out=None, point_range=None, check=False, num_tokens=None):
    """Radar ingest of one sample on the device (tc_radar_build_tokens, HEAD:301-536): the raw
    rows go up as they are (H2D of N x 19 float64), one launch writes the [T,36] token matrix.
    Returns (tokens [1,T,36] -- ``out`` when given, e.g. a pipeline lane's static tensor --,
    count: int32 device tensor with the number of points kept by the range filter,
    pad_mult = N - T + 1), N = ``num_tokens`` (the head's radar_num_tokens; default the reference's 1500).  With T < N at
    most T - 1 points are written (row T - 1 carries pad_mult and stays a pad row); ``check=True`` reads `count` back
    (one D2H sync) and raises when the frame did not fit -- a pipeline checks its lanes' counts after the replay
    instead (FramePipeline.radar_overflow)."""
    from . import radar as R
    N = R.NUM_RADAR_TOKENS if num_tokens is None else int(num_tokens)
    raw, times, start, rr, lr = radar_raw_arrays(frame)
    n = int(start[-1])
    raw_d = torch.from_numpy(raw).to(device, non_blocking=True) if n else None
    times_d = torch.from_numpy(times).to(device, non_blocking=True) if n else None
    if out is None:
        out = torch.empty((1, T, R.NUM_FEATURES), dtype=torch.float32, device=device)
    if tuple(out.shape[-2:]) != (T, R.NUM_FEATURES) or out.numel() != T * R.NUM_FEATURES or not out.is_contiguous():
        raise L.TransCARHipError('out must be a contiguous [1,%d,%d] tensor' % (T, R.NUM_FEATURES))
    count = torch.zeros(1, dtype=torch.int32, device=device)
    pr = (C.c_double * 6)(*[float(v) for v in (point_range or R.POINT_RANGE)])
    L.check(L.lib().tc_radar_build_tokens_n(
        _p(raw_d), _p(times_d), start.ctypes.data_as(C.POINTER(C.c_int)), len(R.RADAR_CHANNELS),
        rr.ctypes.data_as(C.POINTER(C.c_double)), lr.ctypes.data_as(C.POINTER(C.c_double)), pr,
        _p(out), int(T), N, _p(count), L.stream_ptr()), 'tc_radar_build_tokens_n')
    if check:
        radar_check_fits(count, T, N)
    return out, count, N - T + 1


class RadarRawStage:
    """Raw radar of P samples staged for tc_radar_build_tokens_batch: device slabs raw [P,cap,18] f64,
    times [P,cap] f64, descriptors [P] (chan_start / rotations / point range) and count [P], plus pinned host
    mirrors.  ``put(slot, frame)`` packs one sample on the host (no arithmetic beyond quaternion -> rotation
    matrix) and enqueues its three H2D copies on the current stream; ``build(tokens)`` is ONE launch that
    writes the [P,T,36] token tensor (graph-capturable: nothing of a frame is baked into its arguments)."""

    def __init__(self, P, cap, device, point_range=None, num_tokens=None):
        from . import radar as R
        self.P, self.cap, self.device = int(P), int(cap), device
        self.point_range = [float(v) for v in (point_range or R.POINT_RANGE)]
        #: the token count of the head the stage feeds (Detr3DHead.radar_num_tokens)
        self.num_tokens = R.NUM_RADAR_TOKENS if num_tokens is None else int(num_tokens)
        dsz = C.sizeof(L.tc_radar_frame_desc)
        self.raw = torch.zeros((P, cap, 18), dtype=torch.float64, device=device)
        self.times = torch.zeros((P, cap), dtype=torch.float64, device=device)
        self.desc = torch.zeros((P, dsz), dtype=torch.uint8, device=device)
        self.count = torch.zeros(P, dtype=torch.int32, device=device)
        self.h_raw = torch.zeros((P, cap, 18), dtype=torch.float64).pin_memory()
        self.h_times = torch.zeros((P, cap), dtype=torch.float64).pin_memory()
        self.h_desc = torch.zeros((P, dsz), dtype=torch.uint8).pin_memory()
        self.n_raw = [0] * P
        self._copied = [None] * P           # per slot: event behind its last H2D (the pinned mirror is reused)
        for j in range(P):
            self._pack(j, None)
        self.desc.copy_(self.h_desc)

    #: numpy view of tc_radar_frame_desc (same field offsets: checked against the ctypes struct at import)
    DESC_DTYPE = np.dtype([('chan_start', np.int32, (L.TC_MAX_RADAR_CHANNELS + 1,)), ('num_chan', np.int32),
                           ('radar_rot', np.float64, (L.TC_MAX_RADAR_CHANNELS * 9,)), ('lidar_rot', np.float64, (9,)),
                           ('point_range', np.float64, (6,))], align=True)

    def _pack(self, slot, frame):
        from . import radar as R
        d = np.zeros(1, dtype=self.DESC_DTYPE)[0]
        nc = len(R.RADAR_CHANNELS)
        d['num_chan'] = nc
        n = 0
        if frame is not None:
            raw, times, start, rr, lr = radar_raw_arrays(frame)
            n = int(start[-1])
            if n > self.cap:
                raise L.TransCARHipError('radar frame with %d raw points, the stage holds %d per sample' % (n, self.cap))
            if n:
                self.h_raw[slot, :n] = torch.from_numpy(raw)
                self.h_times[slot, :n] = torch.from_numpy(times)
            d['chan_start'][:len(start)] = start
            d['chan_start'][len(start):] = n
            d['radar_rot'][:rr.size] = rr.reshape(-1)
            d['lidar_rot'][:] = lr.reshape(-1)
        d['point_range'][:] = self.point_range
        self.h_desc[slot] = torch.from_numpy(np.frombuffer(d.tobytes(), dtype=np.uint8).copy())
        self.n_raw[slot] = n
        return n

    def put(self, slot, frame):
        """Stage one sample (raw sweeps dict of transcar_amd/radar.py) into slot `slot`: host pack + 3 async H2D."""
        if self._copied[slot] is not None:
            self._copied[slot].synchronize()        # the previous copy out of this slot's pinned mirror has run
        n = self._pack(slot, frame)
        if n:
            self.raw[slot, :n].copy_(self.h_raw[slot, :n], non_blocking=True)
            self.times[slot, :n].copy_(self.h_times[slot, :n], non_blocking=True)
        self.desc[slot].copy_(self.h_desc[slot], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._copied[slot] = ev
        return n

    def put_all(self, frames):
        """Stage samples 0 .. len(frames)-1 at once: every sample packed on the host first, then THREE H2D copies for
        the whole batch (the slabs are contiguous) instead of three per sample -- nine frames per call were 27 copies,
        ~0.15 ms of host time the device spent waiting behind decoder layers 0-3 (round 4)."""
        n = len(frames)
        if n > self.P:
            raise L.TransCARHipError('%d radar frames, the stage holds %d' % (n, self.P))
        for ev in self._copied:
            if ev is not None:
                ev.synchronize()                    # the previous copies out of the pinned mirrors have run
        for slot, frame in enumerate(frames):
            self._pack(slot, frame)
        if n and max(self.n_raw[:n]):
            # whole slots (contiguous slabs: one plain copy each; rows behind a sample's count are never read)
            self.raw[:n].copy_(self.h_raw[:n], non_blocking=True)
            self.times[:n].copy_(self.h_times[:n], non_blocking=True)
        self.desc[:n].copy_(self.h_desc[:n], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._copied = [ev] * n + self._copied[n:]
        return self.n_raw[:n]

    def pack_host(self, frames):
        """Host part of ``put_all`` alone: pack samples 0 .. len(frames)-1 into the pinned mirrors (the caller has made
        sure the copies that last read them are done).  With ``copy_to_device`` as nodes of a captured graph
        (transcar_amd/plugin_graph.py) the H2D copies read whatever the mirrors hold at replay time."""
        if len(frames) > self.P:
            raise L.TransCARHipError('%d radar frames, the stage holds %d' % (len(frames), self.P))
        for slot, frame in enumerate(frames):
            self._pack(slot, frame)
        return self.n_raw[:len(frames)]

    def copy_to_device(self, n=None):
        """The three H2D copies of the first n (default all) samples, whole slots, on the current stream (capturable)."""
        n = self.P if n is None else int(n)
        self.raw[:n].copy_(self.h_raw[:n], non_blocking=True)
        self.times[:n].copy_(self.h_times[:n], non_blocking=True)
        self.desc[:n].copy_(self.h_desc[:n], non_blocking=True)

    def build(self, tokens, n=None):
        """One launch: the first n (default all) samples' raw rows -> tokens[:n] ([n,T,36], contiguous)."""
        from . import radar as R
        n = self.P if n is None else int(n)
        T = int(tokens.shape[1])
        if tokens.dim() != 3 or tokens.shape[0] < n or tokens.shape[2] != R.NUM_FEATURES or not tokens.is_contiguous() \
                or tokens.dtype != torch.float32:
            raise L.TransCARHipError('tokens must be a contiguous fp32 [>=%d,T,%d] tensor' % (n, R.NUM_FEATURES))
        L.check(L.lib().tc_radar_build_tokens_batch_n(_p(self.raw), _p(self.times), _p(self.desc), n, self.cap,
                                                      _p(tokens), T, self.num_tokens, _p(self.count), L.stream_ptr()),
                'tc_radar_build_tokens_batch_n')
        return tokens, self.num_tokens - T + 1


def radar_range_tensor(point_range, device):
    """The radar filter's range as tc_radar_pack_rows_batch takes it: six float64 on the device."""
    return torch.tensor([float(v) for v in point_range], dtype=torch.float64).to(device)


def radar_pack_rows(rows, offsets, T, num_tokens, point_range=None, out=None, count=None, P=None):
    """Feature rows on the device -> tokens (tc_radar_pack_rows_batch; one launch, enqueue-only, graph-capturable).
    rows [total,F] fp32, offsets [P+1] int32 and point_range ([6] float64, or None: no filter), all on the device.
    -> (tokens [P,T,F] -- ``out`` when given --, count [P] int32: rows kept before the truncation, pad_mult)."""
    _chk(rows, 'rows')
    P = int(offsets.numel()) - 1 if P is None else int(P)
    F = int(rows.shape[-1])
    if rows.dim() != 2 or offsets.dtype != torch.int32 or not offsets.is_cuda or not offsets.is_contiguous() \
            or not 1 <= P <= offsets.numel() - 1:
        raise L.TransCARHipError('radar_pack_rows: rows [total,F] fp32 and offsets [P+1] int32 on the GPU')
    if point_range is not None and (point_range.dtype != torch.float64 or not point_range.is_cuda or point_range.numel() != 6):
        raise L.TransCARHipError('radar_pack_rows: point_range must be six float64 on the GPU (radar_range_tensor)')
    if out is None:
        out = torch.empty((P, int(T), F), dtype=torch.float32, device=rows.device)
    if out.dim() != 3 or out.shape[0] < P or tuple(out.shape[1:]) != (int(T), F) or not out.is_contiguous() \
            or out.dtype != torch.float32:
        raise L.TransCARHipError('tokens must be a contiguous fp32 [>=%d,%d,%d] tensor' % (P, T, F))
    if count is None:
        count = torch.empty(P, dtype=torch.int32, device=rows.device)
    L.check(L.lib().tc_radar_pack_rows_batch(_p(rows), int(rows.shape[0]), _p(offsets), P, F, _p(point_range), _p(out),
                                             int(T), int(num_tokens), _p(count), L.stream_ptr()),
            'tc_radar_pack_rows_batch')
    return out, count, int(num_tokens) - int(T) + 1


class RadarRowsStage:
    """Feature rows of P samples staged for tc_radar_pack_rows_batch: a device slab rows [P * cap, F] in which frame slot
    j owns rows j * cap .. (j + 1) * cap - 1 (the fixed offsets a captured graph replays on), and count [P].
    ``put(slot, rows)`` copies one sample's [n,F] rows (device tensor, or pinned host tensor: asynchronous) to the front of
    its slot; the rows of the slot behind them carry NaN coordinates, which the range filter drops like any NaN point --
    so the stage always filters (the head's radar_point_range).  ``build(tokens)`` is ONE launch."""

    def __init__(self, P, cap, in_dims, device, point_range, num_tokens):
        self.P, self.cap, self.in_dims, self.device = int(P), int(cap), int(in_dims), device
        self.num_tokens = int(num_tokens)
        self.rows = torch.full((self.P * self.cap, self.in_dims), float('nan'), dtype=torch.float32, device=device)
        self.offsets = (torch.arange(self.P + 1, dtype=torch.int32) * self.cap).to(device)
        self.range = radar_range_tensor(point_range, device)
        self.count = torch.zeros(self.P, dtype=torch.int32, device=device)
        self.n_rows = [0] * self.P

    def put(self, slot, rows):
        n = int(rows.shape[0])
        if rows.dim() != 2 or rows.shape[1] != self.in_dims or rows.dtype != torch.float32:
            raise L.TransCARHipError('radar_rows must be an fp32 [n,%d] tensor (radar_in_dims=%d), got %s %s'
                                     % (self.in_dims, self.in_dims, tuple(rows.shape), rows.dtype))
        if n > self.cap:
            raise L.TransCARHipError('radar frame with %d rows, the stage holds %d per sample' % (n, self.cap))
        dst = self.rows[slot * self.cap:(slot + 1) * self.cap]
        if n:
            dst[:n].copy_(rows, non_blocking=True)
        if self.n_rows[slot] > n:                    # what the slot's previous frame left behind the new one
            dst[n:self.n_rows[slot], :3] = float('nan')
        self.n_rows[slot] = n
        return n

    def build(self, tokens, n=None):
        """One launch: the first n (default all) slots' rows -> tokens[:n] ([n,T,F], contiguous)."""
        n = self.P if n is None else int(n)
        return radar_pack_rows(self.rows, self.offsets, int(tokens.shape[1]), self.num_tokens, self.range, out=tokens,
                               count=self.count, P=n)[::2]


def radar_tokens_T(n_points, granule=64, num_tokens=None):
    """Token count for frames of at most n_points kept (or raw) points: the smallest multiple of `granule`
    that holds them plus the pad row, at most the head's token count (default 1500; radar.pack_tokens's rule)."""
    from . import radar as R
    N = R.NUM_RADAR_TOKENS if num_tokens is None else int(num_tokens)
    return min(N, ((min(int(n_points), N) + 1 + granule - 1) // granule) * granule)


def radar_check_fits(count, T, num_tokens=None):
    """Raise when the device ingest kept more points than a [T,F] token matrix can hold
    (T < N: T - 1 points + the pad row; T = N, the head's token count: the reference's own truncation)."""
    from . import radar as R
    N = R.NUM_RADAR_TOKENS if num_tokens is None else int(num_tokens)
    n = int(count.max().item())
    if T < N and n > T - 1:
        raise L.TransCARHipError('radar ingest: %d points kept, T=%d holds %d (+ the pad row): use a '
                                 'larger T (up to %d)' % (n, T, T - 1, N))


def box_decode_topk(cls_scores, bbox_preds, post_center_range, max_num=300, path=0):
    """NMSFreeCoder.decode_single + z-shift (CODER:39-90, HEAD:1018) for a
    batch: fixed-size outputs + a validity mask.  path: 0 the kernel the shape
    asks for, 1 the in-register kernel, 2 the streaming kernel (the same bits
    where both apply)."""
    _chk(cls_scores, 'cls_scores'); _chk(bbox_preds, 'bbox_preds')
    B, Q, ncls = cls_scores.shape
    dev = cls_scores.device
    boxes = torch.empty((B, max_num, 9), dtype=torch.float32, device=dev)
    scores = torch.empty((B, max_num), dtype=torch.float32, device=dev)
    labels = torch.empty((B, max_num), dtype=torch.int32, device=dev)
    valid = torch.empty((B, max_num), dtype=torch.uint8, device=dev)
    L.check(L.lib().tc_box_decode_topk_path(
        _p(cls_scores), _p(bbox_preds), B, Q, ncls, bbox_preds.shape[-1],
        max_num, L.f6(post_center_range), _p(boxes), _p(scores), _p(labels),
        _p(valid), None, 0, L.stream_ptr(), int(path)), 'tc_box_decode_topk')
    return boxes, scores, labels, valid


def box_decode_kept(cls_scores, bbox_preds, post_center_range, max_num=300, score_threshold=None, z_shift=True,
                    count_out=None, out=None, path=0):
    """NMSFreeCoder.decode_single for a batch (tc_box_decode_kept): the kept rows (inside post_center_range, above
    the score threshold) compacted in score order -> boxes [B,max_num,9], scores [B,max_num], labels [B,max_num]
    (int64) and count [B] (int32, device); rows beyond count[b] are not written.  path: as box_decode_topk."""
    _chk(cls_scores, 'cls_scores'); _chk(bbox_preds, 'bbox_preds')
    B, Q, ncls = cls_scores.shape
    dev = cls_scores.device
    if out is not None:                 # (boxes [B,max_num,9] f32, scores [B,max_num] f32, labels [B,max_num] i64): static buffers of a graph
        boxes, scores, labels = out
        if tuple(boxes.shape) != (B, max_num, 9) or tuple(scores.shape) != (B, max_num) or tuple(labels.shape) != (B, max_num) \
                or labels.dtype != torch.int64 or not (boxes.is_contiguous() and scores.is_contiguous() and labels.is_contiguous()):
            raise L.TransCARHipError('box_decode_kept: out tensors of the wrong shape / dtype')
    else:
        boxes = torch.empty((B, max_num, 9), dtype=torch.float32, device=dev)
        scores = torch.empty((B, max_num), dtype=torch.float32, device=dev)
        labels = torch.empty((B, max_num), dtype=torch.int64, device=dev)
    # count_out: an int32 device tensor of B elements to write the counts to (Detr3DHead.get_bboxes: the words behind
    # the head's range status, so that ONE small D2H reads both)
    count = count_out if count_out is not None else torch.empty((B,), dtype=torch.int32, device=dev)
    use_thr = bool(score_threshold)                   # CODER:73: `if self.score_threshold:` -- None and 0 are off
    L.check(L.lib().tc_box_decode_kept_path(
        _p(cls_scores), _p(bbox_preds), B, Q, ncls, bbox_preds.shape[-1], max_num, L.f6(post_center_range),
        float(score_threshold) if use_thr else 0.0, int(use_thr), int(bool(z_shift)),
        _p(boxes), _p(scores), _p(labels), _p(count), L.stream_ptr(), int(path)), 'tc_box_decode_kept')
    return boxes, scores, labels, count


class _Lidar2ImgStaging:
    """Host -> device staging of the per-frame projection matrices (XFMR:382-386) for the plugin entry: a ring of
    pinned [B,N,4,4] buffers (one asynchronous H2D on the caller's stream, no pageable bounce), and no copy at all
    when the matrices are the ones staged last (a static rig replayed, benchmark loops).  The device tensors stay
    inside the head (``Detr3DHead.forward``): nobody else can write to a cached one."""
    RING = 8

    def __init__(self):
        import threading
        self.slots = {}        # (device, shape) -> [pinned tensors, events, next]
        self.last = {}         # device -> (host copy, device tensor, stream id, event)
        self.lock = threading.Lock()      # forwards from several host threads (one per stream) share this object

    def get(self, l2i, device):
        with self.lock:
            return self._get(l2i, device)

    def _get(self, l2i, device):
        key = str(device)
        cur = torch.cuda.current_stream(device)
        hit = self.last.get(key)
        if hit is not None and hit[0].shape == l2i.shape and np.array_equal(hit[0], l2i):
            if hit[2] != cur.cuda_stream:
                cur.wait_event(hit[3])
                # a consumer on ANOTHER stream: the caching allocator must not hand the tensor's memory out again (it
                # is replaced on the next miss) before that stream's work has finished with it
                hit[1].record_stream(cur)
            return hit[1]
        ring = self.slots.get((key, l2i.shape))
        if ring is None:
            ring = self.slots[(key, l2i.shape)] = [
                [torch.empty(l2i.shape, dtype=torch.float32).pin_memory() for _ in range(self.RING)],
                [None] * self.RING, 0]
        i = ring[2]
        ring[2] = (i + 1) % self.RING
        if ring[1][i] is not None:
            ring[1][i].synchronize()               # the copy that last read this pinned buffer (8 frames ago)
        ring[0][i].numpy()[...] = l2i
        out = torch.empty(l2i.shape, dtype=torch.float32, device=device)
        out.copy_(ring[0][i], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(cur)
        ring[1][i] = ev
        self.last[key] = (l2i, out, cur.cuda_stream, ev)
        return out


_l2i_staging = _Lidar2ImgStaging()


def lidar2img_tensor(img_metas, device, staged=False):
    """XFMR:382-386: stack img_metas[i]['lidar2img'] -> [B,N,4,4] fp32 on `device`.
    staged: through the head's pinned staging ring / last-matrices cache (the result must not be written to)."""
    l2i = np.asarray([m['lidar2img'] for m in img_metas], dtype=np.float32)
    device = torch.device(device)
    if not staged or device.type != 'cuda':
        return torch.from_numpy(l2i).to(device).contiguous()
    return _l2i_staging.get(l2i, device)
