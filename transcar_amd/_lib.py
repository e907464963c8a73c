"""ctypes binding of the C ABI in include/transcar_hip.h.

The HIP library is the product; there is no CPU fallback.  ``lib()`` raises
``TransCARHipError`` if ``transcar_amd/lib/libtranscar_hip.so`` is missing
(build it with ``python -c 'import __graft_entry__ as g; g.build()'`` or
``make -C transcar_amd/csrc``), and every call checks the returned status.
"""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
#: TRANSCAR_HIP_LIB selects another build of the same ABI.  The STAMPS debug build
#: (`make STAMPS=1`: s_memtime stamps and the TRANSCAR_CHAIN_DBG timing switches, which
#: produce WRONG results) is refused unless TRANSCAR_ALLOW_STAMPS=1 is set as well
#: (tools/chain_stamps.py); it is built under build/hip_stamps/, not into transcar_amd/lib/,
#: and is never the product.
LIB_PATH = os.environ.get('TRANSCAR_HIP_LIB') or os.path.join(_HERE, 'lib', 'libtranscar_hip.so')

TC_MAX_LEVELS = 4      # FPN levels of tc_feats_nhwc / Detr3DCrossAtten.num_levels (include/transcar_hip.h)
TC_MAX_LAYERS = 8
TC_MAX_RADAR_LAYERS = 3
TC_ABI_VERSION = 13

c_fp = C.c_void_p      # device pointers travel as integers


class TransCARHipError(RuntimeError):
    pass


# num_cams * num_levels * num_points of Detr3DCrossAtten (include/transcar_hip.h)
TC_MAX_CAM_LOGITS = 256


def check_num_points(num_points, num_cams, num_levels):
    """The library's limit on Detr3DCrossAtten.num_points, checked before
    anything is packed or launched."""
    if int(num_points) < 1 or num_cams * num_levels * int(num_points) > TC_MAX_CAM_LOGITS:
        raise TransCARHipError(
            'Detr3DCrossAtten(HIP): num_points=%r is not supported (num_points >= 1 and '
            'num_cams * num_levels * num_points = %d * %d * num_points <= %d)'
            % (num_points, num_cams, num_levels, TC_MAX_CAM_LOGITS))


# cameras per frame of a head and of the camera-sampling entries (include/transcar_hip.h)
TC_MAX_CAMS = 16


def check_num_cams(num_cams):
    """The library's limit on Detr3DCrossAtten.num_cams (1 .. TC_MAX_CAMS: the sampling kernels give a row one lane
    per camera, 16 lanes), checked before anything is packed or launched.  Returns the count."""
    if isinstance(num_cams, bool) or not isinstance(num_cams, int) or not 1 <= num_cams <= TC_MAX_CAMS:
        raise TransCARHipError(
            'Detr3DCrossAtten(HIP): num_cams=%r is not supported (an int, 1 .. %d cameras)' % (num_cams, TC_MAX_CAMS))
    return num_cams


def check_frame_cams(num_cams, lidar2img_cams, B=None, feat_rows=None):
    """A frame against the head that takes it: lidar2img carries `lidar2img_cams` matrices per sample and every feature
    map `feat_rows` leading rows (an iterable, one per level); the kernels index both by the head's num_cams, so a
    frame of another rig is refused before any launch."""
    if lidar2img_cams is not None and int(lidar2img_cams) != num_cams:
        raise TransCARHipError(
            'Detr3DHead(HIP): the frame has %d lidar2img matrices per sample, the head was built for num_cams=%d'
            % (lidar2img_cams, num_cams))
    for lvl, rows in enumerate(feat_rows or ()):
        if int(rows) != B * num_cams:
            raise TransCARHipError(
                'Detr3DHead(HIP): feature map %d has %d images, B * num_cams = %d * %d = %d expected'
                % (lvl, rows, B, num_cams, B * num_cams))


def check_num_levels(num_levels):
    """The library's limit on Detr3DCrossAtten.num_levels (1 .. TC_MAX_LEVELS),
    checked before anything is packed or launched."""
    if int(num_levels) != num_levels or not 1 <= int(num_levels) <= TC_MAX_LEVELS:
        raise TransCARHipError(
            'Detr3DCrossAtten(HIP): num_levels=%r is not supported (1 .. %d FPN levels)'
            % (num_levels, TC_MAX_LEVELS))


# heads of the decoder's MultiheadAttention at embed_dims 256: head dimension 64, 32, 16 (include/transcar_hip.h)
TC_NUM_HEADS = (4, 8, 16)
# default heads of the radar fusion attention: nn.MultiheadAttention(embed_dims, 8) in the reference, whatever the decoder
# uses; Detr3DHead(radar_num_heads=) takes TC_NUM_HEADS too
TC_RADAR_HEADS = 8


def pack_num_heads(decoder_heads, radar_heads=TC_RADAR_HEADS):
    """tc_head_weights.num_heads (TC_NUM_HEADS_PACK): the decoder's count in the lower 16 bits, the radar fusion
    attention's in the upper 16 -- left 0 (= TC_RADAR_HEADS) at the default, which keeps the default head's struct as it was."""
    return decoder_heads | ((radar_heads << 16) if radar_heads != TC_RADAR_HEADS else 0)

# num_classes of a head (tc_head_weights, tc_decoder_heads)
TC_MAX_CLASSES = 32

# box decode: num_query * num_classes and max_num of the in-register kernel and of the streaming kernel that takes the
# shapes beyond it (include/transcar_hip.h); path of tc_box_decode_*_path
TC_BOX_DECODE_MAX_SCORES, TC_BOX_DECODE_MAX_NUM = 12288, 512
TC_BOX_DECODE_STREAM_MAX_SCORES, TC_BOX_DECODE_STREAM_MAX_NUM = 1 << 20, 2048
TC_DECODE_AUTO, TC_DECODE_REGISTERS, TC_DECODE_STREAM = 0, 1, 2

# Hungarian assignment on the device: num_query and boxes per sample of tc_lsa_assign_ws, and of the kernel that keeps a
# sample's costs in LDS (tc_lsa_assign / _ex; no workspace); path of tc_lsa_assign_ws (include/transcar_hip.h)
TC_LSA_MAX_QUERIES, TC_LSA_MAX_GT = 4096, 512
TC_LSA_SMALL_MAX_QUERIES, TC_LSA_SMALL_MAX_GT = 1024, 128
TC_LSA_AUTO, TC_LSA_SMALL, TC_LSA_LARGE = 0, 1, 2


def lsa_large_workspace_bytes(num_outputs, B, Q, Gmax):
    """The workspace of tc_lsa_assign_ws's large kernel, whatever the shape: the transposed costs [P][Gmax][Qpad]
    (float, Qpad = Q rounded up to 64) and one flag word per problem, each rounded up to 256 bytes.
    tc_lsa_workspace_bytes returns this for a shape beyond the small kernel's limits and 0 within them."""
    P, qpad = num_outputs * B, (Q + 63) // 64 * 64
    return (P * Gmax * qpad * 4 + 255) // 256 * 256 + (P * 4 + 255) // 256 * 256


def check_num_heads(num_heads):
    """The library's limit on the decoder MultiheadAttention's num_heads (4, 8
    or 16 at embed_dims 256), checked before anything is packed or launched."""
    if isinstance(num_heads, bool) or not isinstance(num_heads, int) or num_heads not in TC_NUM_HEADS:
        raise TransCARHipError(
            'MultiheadAttention(HIP): num_heads=%r is not supported (4, 8 or 16 heads at embed_dims 256: '
            'head dimension 64, 32 or 16)' % (num_heads,))


# tc_head_weights.ffn_dims, the decoder layers' feedforward_channels: what the fused row chains run (include/transcar_hip.h);
# the width of the fusion layers' FFN, rf_linear1 / rf_linear2, whatever the decoder's is
TC_FFN_DIMS_MIN, TC_FFN_DIMS_MAX, TC_FFN_DIMS_STEP = 256, 2048, 256
TC_RADAR_FFN_DIMS = 512


def check_ffn_dims(ffn_dims):
    """The library's limit on a decoder layer's feedforward_channels (tc_head_weights.ffn_dims: a multiple of 256 from
    256 to 2048 -- the fused chains run the FFN in chunks of 512 hidden units, the last one 256 or 512 wide), checked
    before anything is built, packed or launched.  Returns the width."""
    f = ffn_dims
    if (isinstance(f, bool) or not isinstance(f, int) or not TC_FFN_DIMS_MIN <= f <= TC_FFN_DIMS_MAX
            or f % TC_FFN_DIMS_STEP != 0):
        raise TransCARHipError(
            'DetrTransformerDecoderLayer(HIP): feedforward_channels, ffn_dims=%r, is not supported (the accepted set: '
            'multiples of %d from %d to %d)' % (f, TC_FFN_DIMS_STEP, TC_FFN_DIMS_MIN, TC_FFN_DIMS_MAX))
    return f


def check_radar_num_heads(radar_num_heads):
    """The library's limit on the head count of the radar fusion attention (rf_multihead_attn{,2,3}: 4, 8 or 16 at
    embed_dims 256), checked before anything is built, packed or launched.  Returns the count."""
    h = radar_num_heads
    if isinstance(h, bool) or not isinstance(h, int) or h not in TC_NUM_HEADS:
        raise TransCARHipError(
            'Detr3DHead(HIP): radar_num_heads=%r is not supported (4, 8 or 16 heads at embed_dims 256: '
            'head dimension 64, 32 or 16)' % (h,))
    return h


def check_num_classes(num_classes):
    """The library's limit on a head's num_classes (1 .. 32: the class heads of the
    row chains take one or two 16-column sub-tiles), checked before anything is
    packed or launched."""
    if isinstance(num_classes, bool) or not isinstance(num_classes, int) or not 1 <= num_classes <= TC_MAX_CLASSES:
        raise TransCARHipError(
            'Detr3DHead(HIP): num_classes=%r is not supported (1 .. %d classes)' % (num_classes, TC_MAX_CLASSES))


def check_num_fusion_layers(num_fusion_layers):
    """The library's limit on the depth of the radar fusion stack (1 .. TC_MAX_RADAR_LAYERS
    layers; the reference builds 3), checked before anything is built, packed or launched.
    Returns the depth.  No fusion layer at all is what ``outputs='camera'`` is for."""
    n = num_fusion_layers
    if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= TC_MAX_RADAR_LAYERS:
        raise TransCARHipError(
            "Detr3DHead(HIP): num_fusion_layers=%r is not supported (1 .. %d radar fusion layers; a head without "
            "the fusion stack is outputs='camera')" % (n, TC_MAX_RADAR_LAYERS))
    return n


# The distance gate of the radar fusion layers (include/transcar_hip.h, TC_RADAR_GATE_CIRCLE): a (radius_min, radius_max)
# pair per layer; radius_min == TC_RADAR_GATE_CIRCLE encodes one circle of the fixed radius radius_max, edge inside.
# A radius lies in [TC_RADAR_RADIUS_MIN, TC_RADAR_RADIUS_MAX] metres: below is under the sensor's resolution, beyond
# a gate is no longer local (and the kernels' threshold search is checked on this range).
TC_RADAR_GATE_CIRCLE = -1.0
TC_RADAR_RADIUS_MIN, TC_RADAR_RADIUS_MAX = 0.125, 16.0
RADAR_GATE_TYPES = ('three_circle', 'circle')
#: the three-circle clamp pairs of the reference's three fusion layers (HEAD:567, 635, 693)
RADAR_RADII = ((1.0, 2.0), (1.0, 2.0), (0.5, 1.0))


def _gate_radius(v, gate):
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise TransCARHipError('Detr3DHead(HIP): radar_gate=%r: radius %r is not a number' % (gate, v))
    v = float(v)
    if not TC_RADAR_RADIUS_MIN <= v <= TC_RADAR_RADIUS_MAX:        # (a NaN fails both comparisons)
        raise TransCARHipError('Detr3DHead(HIP): radar_gate=%r: radius %r is outside %g .. %g m'
                               % (gate, v, TC_RADAR_RADIUS_MIN, TC_RADAR_RADIUS_MAX))
    return v


def check_radar_gate(radar_gate, num_fusion_layers=TC_MAX_RADAR_LAYERS):
    """The distance gate of the radar fusion layers, checked before anything is built, packed or launched; returns it
    normalised: ``dict(type=..., radii=(one entry per fusion layer))``.

    * ``None`` or ``dict(type='three_circle')``: three circles per query (centre, front and rear) of the radius
      clamp(length / 2, rmin, rmax), a token attended iff ``dist < radius`` for any (HEAD:549-571), with the reference's
      pairs RADAR_RADII; ``radii=[(rmin, rmax), ...]`` sets other pairs.
    * ``dict(type='circle', radii=[R, ...])``: one circle of radius R at the gate centre, a token attended iff not
      ``dist > R`` (the edge is inside).

    ``radii`` has one entry per fusion layer; a list of TC_MAX_RADAR_LAYERS is also taken by a shallower head, which
    uses its first entries."""
    n = check_num_fusion_layers(num_fusion_layers)
    gate = radar_gate
    if gate is None:
        gate = dict(type='three_circle')
    if not isinstance(gate, dict) or set(gate) - {'type', 'radii'} or gate.get('type') not in RADAR_GATE_TYPES:
        raise TransCARHipError("Detr3DHead(HIP): radar_gate=%r is not supported (None, dict(type='three_circle'[, radii="
                               "[(rmin, rmax), ...]]) or dict(type='circle', radii=[R, ...]))" % (radar_gate,))
    kind, radii = gate['type'], gate.get('radii')
    if radii is None and kind == 'three_circle':
        radii = RADAR_RADII
    if not isinstance(radii, (list, tuple)) or len(radii) not in (n, TC_MAX_RADAR_LAYERS):
        raise TransCARHipError('Detr3DHead(HIP): radar_gate=%r: radii needs one entry per fusion layer (%d, or %d of which '
                               'the first %d are used)' % (radar_gate, n, TC_MAX_RADAR_LAYERS, n))
    out = []
    for entry in radii[:n]:
        if kind == 'circle':
            out.append(_gate_radius(entry, radar_gate))
            continue
        if not isinstance(entry, (list, tuple)) or len(entry) != 2:
            raise TransCARHipError('Detr3DHead(HIP): radar_gate=%r: %r is not a (rmin, rmax) pair' % (radar_gate, entry))
        rmin, rmax = (_gate_radius(v, radar_gate) for v in entry)
        if rmin > rmax:
            raise TransCARHipError('Detr3DHead(HIP): radar_gate=%r: rmin %r is above rmax %r' % (radar_gate, rmin, rmax))
        out.append((rmin, rmax))
    return dict(type=kind, radii=tuple(out))


def radar_gate_pairs(gate):
    """The (radius_min, radius_max) pairs of a normalised gate (check_radar_gate) as the C boundary takes them."""
    if gate['type'] == 'circle':
        return [(TC_RADAR_GATE_CIRCLE, r) for r in gate['radii']]
    return [tuple(p) for p in gate['radii']]


# The radar input of a head (include/transcar_hip.h): the token count it attends over, the features per token and the
# range of the radar filter.  The defaults are the reference's constants (HEAD:526, 183, 304).
TC_RADAR_TOKENS_REF = 1500
TC_MIN_RADAR_TOKENS, TC_MAX_RADAR_TOKENS = 64, 4096
TC_MAX_RADAR_IN_DIMS = 64
RADAR_IN_DIMS_REF = 36
RADAR_POINT_RANGE_REF = (-51.2, -51.2, -5.0, 51.2, 51.2, 3.0)


def check_radar_input(radar_num_tokens=TC_RADAR_TOKENS_REF, radar_in_dims=RADAR_IN_DIMS_REF, radar_point_range=None):
    """The library's limits on a head's radar input, checked before anything is built, packed or launched; returns
    (radar_num_tokens, radar_in_dims, radar_point_range as six floats).

    * ``radar_num_tokens``: TC_MIN_RADAR_TOKENS .. TC_MAX_RADAR_TOKENS tokens attended per frame (a frame's first N kept
      points; the reference's 1500, HEAD:526-530);
    * ``radar_in_dims``: 4, 8, .. TC_MAX_RADAR_IN_DIMS features per token, columns 0..2 being x, y, z (36 in the reference);
    * ``radar_point_range``: (x0, y0, z0, x1, y1, z1) of the radar filter, finite with x0 < x1, y0 < y1, z0 < z1; None is the
      reference's constant (HEAD:304) -- it does not follow pc_range."""
    n, f, rng = radar_num_tokens, radar_in_dims, radar_point_range
    if isinstance(n, bool) or not isinstance(n, int) or not TC_MIN_RADAR_TOKENS <= n <= TC_MAX_RADAR_TOKENS:
        raise TransCARHipError('Detr3DHead(HIP): radar_num_tokens=%r is not supported (%d .. %d tokens)'
                               % (n, TC_MIN_RADAR_TOKENS, TC_MAX_RADAR_TOKENS))
    if isinstance(f, bool) or not isinstance(f, int) or not 4 <= f <= TC_MAX_RADAR_IN_DIMS or f % 4:
        raise TransCARHipError('Detr3DHead(HIP): radar_in_dims=%r is not supported (4, 8, .. %d features per token)'
                               % (f, TC_MAX_RADAR_IN_DIMS))
    if rng is None:
        rng = RADAR_POINT_RANGE_REF
    ok = isinstance(rng, (list, tuple)) and len(rng) == 6 and \
        all(isinstance(v, (int, float)) and not isinstance(v, bool) for v in rng)
    if ok:
        rng = tuple(float(v) for v in rng)
        ok = all(abs(v) < float('inf') for v in rng) and all(rng[i] < rng[3 + i] for i in range(3))   # (a NaN fails both)
    if not ok:
        raise TransCARHipError('Detr3DHead(HIP): radar_point_range=%r is not supported ((x0, y0, z0, x1, y1, z1), finite, '
                               'x0 < x1, y0 < y1, z0 < z1)' % (radar_point_range,))
    return n, f, rng


def cam_pregather_supported(embed_dims, num_levels, num_cams):
    """The shapes the camera pre-gather (tc_head_options.cam_pregather) runs:
    C = 256, 4 levels, at most 8 cameras.  Others take the chain's own gather,
    with bit-identical outputs; asking the library for the pre-gather on them
    is an error."""
    return embed_dims == 256 and num_levels == TC_MAX_LEVELS and num_cams <= 8


TC_MAX_RADAR_CHANNELS = 8
TC_SQ_NORM_PARTIALS = 256


class tc_radar_frame_desc(C.Structure):
    _fields_ = [('chan_start', C.c_int * (TC_MAX_RADAR_CHANNELS + 1)), ('num_chan', C.c_int),
                ('radar_rot', C.c_double * (TC_MAX_RADAR_CHANNELS * 9)), ('lidar_rot', C.c_double * 9),
                ('point_range', C.c_double * 6)]


class tc_linear(C.Structure):
    _fields_ = [('w', c_fp), ('b', c_fp)]


class tc_lnorm(C.Structure):
    _fields_ = [('g', c_fp), ('b', c_fp)]


class tc_pos_encoder(C.Structure):
    _fields_ = [('l0', tc_linear), ('n1', tc_lnorm), ('l3', tc_linear),
                ('n4', tc_lnorm)]


class tc_cls_branch(C.Structure):
    _fields_ = [('l0', tc_linear), ('n1', tc_lnorm), ('l3', tc_linear),
                ('n4', tc_lnorm), ('l6', tc_linear)]


class tc_reg_branch(C.Structure):
    _fields_ = [('l0', tc_linear), ('l2', tc_linear), ('l4', tc_linear)]


class tc_mha(C.Structure):
    _fields_ = [('in_proj', tc_linear), ('out_proj', tc_linear)]


class tc_decoder_layer(C.Structure):
    _fields_ = [('self_attn', tc_mha), ('norm0', tc_lnorm),
                ('attention_weights', tc_linear), ('output_proj', tc_linear),
                ('position_encoder', tc_pos_encoder), ('norm1', tc_lnorm),
                ('ffn0', tc_linear), ('ffn1', tc_linear), ('norm2', tc_lnorm),
                ('reg', tc_reg_branch), ('packed16_delta', C.c_size_t)]


class tc_radar_layer(C.Structure):
    _fields_ = [('attn', tc_mha), ('norm2', tc_lnorm), ('linear1', tc_linear),
                ('linear2', tc_linear), ('norm3', tc_lnorm),
                ('final_cls', tc_cls_branch), ('final_reg', tc_reg_branch),
                ('radius_min', C.c_float), ('radius_max', C.c_float), ('packed16_delta', C.c_size_t)]


class tc_head_weights(C.Structure):
    _fields_ = [('abi_version', C.c_int),
                ('num_query', C.c_int), ('embed_dims', C.c_int),
                ('num_heads', C.c_int), ('ffn_dims', C.c_int),
                ('num_layers', C.c_int),
                ('num_cams', C.c_int), ('num_levels', C.c_int),
                ('num_classes', C.c_int), ('code_size', C.c_int),
                ('radar_in_dims', C.c_int), ('num_radar_layers', C.c_int),
                ('num_radar_tokens_ref', C.c_int),
                ('pc_range', C.c_float * 6),
                ('query_embedding', c_fp),
                ('reference_points', tc_linear),
                ('layers', tc_decoder_layer * TC_MAX_LAYERS),
                ('radar_position_encoder', tc_pos_encoder),
                ('radar_feat0', tc_linear), ('radar_feat2', tc_linear),
                ('radar_feat4', tc_linear),
                ('radar', tc_radar_layer * TC_MAX_RADAR_LAYERS),
                ('l0_init_reference', c_fp), ('l0_attn_out', c_fp), ('packed16_delta', C.c_size_t),
                ('num_points', C.c_int)]


class tc_decoder_heads(C.Structure):
    """cls_branches / reg_branches of the decoder levels (tc_decoder_heads_pack, tc_decoder_outputs_fwd)."""
    _fields_ = [('abi_version', C.c_int), ('num_levels', C.c_int), ('embed_dims', C.c_int),
                ('num_classes', C.c_int), ('code_size', C.c_int),
                ('pc_range', C.c_float * 6),
                ('cls', tc_cls_branch * TC_MAX_LAYERS), ('reg', tc_reg_branch * TC_MAX_LAYERS),
                ('packed16_delta', C.c_size_t)]


class tc_feats_nhwc(C.Structure):
    _fields_ = [('num_levels', C.c_int),
                ('data', c_fp * TC_MAX_LEVELS),
                ('H', C.c_int * TC_MAX_LEVELS),
                ('W', C.c_int * TC_MAX_LEVELS)]


class tc_head_aux(C.Structure):
    _fields_ = [('inter_states', c_fp), ('init_reference', c_fp),
                ('inter_references', c_fp), ('radar_hit_counts', c_fp),
                ('last_box', c_fp), ('sample_pairs', c_fp)]


class tc_head_options(C.Structure):
    _fields_ = [('chain_tile_rows', C.c_int), ('unfused', C.c_int),
                ('last_level_cls_only', C.c_int), ('reuse_radar_kv', C.c_int),
                ('decoder_dropout_p', C.c_float), ('radar_row_order', C.c_int),
                ('dropout_seed', C.c_ulonglong), ('phase', C.c_int), ('matrix_path', C.c_int),
                ('dropout_seed_stride', C.c_ulonglong), ('range_status', c_fp), ('cam_pregather', C.c_int),
                ('cam_pregather_ws', c_fp), ('cam_pregather_bytes', C.c_size_t)]


TC_MATRIX_AUTO, TC_MATRIX_F32, TC_MATRIX_F16X2 = 0, 1, 2


_P = C.POINTER
_i, _f, _sz, _vp = C.c_int, C.c_float, C.c_size_t, C.c_void_p

#: name -> (restype, argtypes); mirrors include/transcar_hip.h one to one
SIGNATURES = {
    'tc_abi_version': (_i, []),
    'tc_last_error': (C.c_char_p, []),
    'tc_chain_tile_rows': (_i, [_i, _i, _i]),
    'tc_device_count': (_i, []),
    'tc_nchw_to_nhwc': (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    'tc_nchw_to_nhwc_levels': (_i, [_P(_vp), _P(_vp), _i, _i, _i, _P(_i), _P(_i), _vp]),
    'tc_radar_build_tokens': (_i, [_vp, _vp, _P(_i), _i, _P(C.c_double), _P(C.c_double),
                                   _P(C.c_double), _vp, _i, _vp, _vp]),
    'tc_radar_build_tokens_batch': (_i, [_vp, _vp, _vp, _i, _i, _vp, _i, _vp, _vp]),
    'tc_radar_build_tokens_n': (_i, [_vp, _vp, _P(_i), _i, _P(C.c_double), _P(C.c_double),
                                     _P(C.c_double), _vp, _i, _i, _vp, _vp]),
    'tc_radar_build_tokens_batch_n': (_i, [_vp, _vp, _vp, _i, _i, _vp, _i, _i, _vp, _vp]),
    'tc_radar_pack_rows_batch': (_i, [_vp, _i, _vp, _i, _i, _vp, _vp, _i, _i, _vp, _vp]),
    'tc_linear_fwd': (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    'tc_add_layernorm_fwd': (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    'tc_refine_reference_fwd': (_i, [_vp, _i, _vp, _vp, _i, _vp]),
    'tc_cam_sample_fuse_fwd': (_i, [_P(tc_feats_nhwc), _i, _i, _i, _i, _vp,
                                    _vp, _vp, _P(_f), _f, _f, _vp, _vp, _vp,
                                    _vp]),
    'tc_cam_sample_fuse_points_fwd': (_i, [_P(tc_feats_nhwc), _i, _i, _i, _i, _i,
                                           _vp, _vp, _vp, _P(_f), _f, _f, _vp,
                                           _vp, _vp, _vp]),
    'tc_cross_atten_workspace_bytes': (_sz, [_i, _i, _i, _i, _i]),
    'tc_cross_atten_points_workspace_bytes': (_sz, [_i, _i, _i, _i, _i, _i]),
    'tc_cross_atten_points_fwd': (_i, [_P(tc_linear), _P(tc_linear),
                                       _P(tc_pos_encoder), _P(tc_feats_nhwc),
                                       _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp,
                                       _P(_f), _f, _f, _vp, _vp, _sz, _vp]),
    'tc_cross_atten_fwd': (_i, [_P(tc_linear), _P(tc_linear),
                                _P(tc_pos_encoder), _P(tc_feats_nhwc), _i, _i,
                                _i, _i, _vp, _vp, _vp, _vp, _P(_f), _f, _f,
                                _vp, _vp, _sz, _vp]),
    'tc_self_attn_workspace_bytes': (_sz, [_i, _i, _i]),
    'tc_self_attn_fwd': (_i, [_P(tc_mha), _vp, _vp, _vp, _i, _i, _i, _i, _vp,
                              _sz, _vp]),
    'tc_decoder_layer_tail_fwd': (_i, [_P(tc_decoder_layer), _P(tc_linear),
                                       _P(tc_feats_nhwc), _i, _i, _i, _i, _vp,
                                       _vp, _vp, _vp, _vp, _P(_f), _f, _f, _vp,
                                       _vp, _vp, _vp, _i, _i, _vp]),
    'tc_decoder_layer_tail_fwd_ffn': (_i, [_P(tc_decoder_layer), _P(tc_linear),
                                           _P(tc_feats_nhwc), _i, _i, _i, _i, _vp,
                                           _vp, _vp, _vp, _vp, _P(_f), _f, _f, _vp,
                                           _vp, _vp, _vp, _i, _i, _i, _vp]),
    'tc_sdpa_fwd': (_i, [_vp, _vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _vp]),
    'tc_sdpa_f16x2_workspace_bytes': (_sz, [_i, _i, _i]),
    'tc_sdpa_fwd_f16x2': (_i, [_vp, _vp, _i, _vp, _i, _i, _i, _i, _vp, _sz, _vp]),
    'tc_sdpa_fwd_hd': (_i, [_vp, _vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _i, _vp]),
    'tc_sdpa_fwd_f16x2_hd': (_i, [_vp, _vp, _i, _vp, _i, _i, _i, _i, _i, _vp]),
    'tc_radar_xattn_workspace_bytes': (_sz, [_i, _i, _i, _i]),
    'tc_radar_gate_selfcheck': (_i, [_i, C.c_ulonglong, _vp, _vp]),
    'tc_radar_gate_selfcheck_range': (_i, [_i, C.c_ulonglong, C.c_float, C.c_float, _i, _vp, _vp]),
    'tc_rowops_selfcheck': (_i, [_i, C.c_ulonglong, _vp, _vp]),
    'tc_radar_gated_xattn_fwd': (_i, [_P(tc_mha), _vp, _vp, _vp, _i, _vp, _vp,
                                      _i, _i, _i, _i, _i, _i, _f, _f, _vp,
                                      _vp, _vp, _sz, _vp]),
    'tc_radar_fusion_fwd': (_i, [_P(tc_head_weights), _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i,
                                 _vp, _vp, _vp, _P(tc_head_options), _vp, _sz, _vp]),
    'tc_box_decode_workspace_bytes': (_sz, [_i, _i, _i]),
    'tc_box_decode_topk': (_i, [_vp, _vp, _i, _i, _i, _i, _i, _P(_f), _vp,
                                _vp, _vp, _vp, _vp, _sz, _vp]),
    'tc_box_decode_kept': (_i, [_vp, _vp, _i, _i, _i, _i, _i, _P(_f), _f, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    'tc_box_decode_topk_path': (_i, [_vp, _vp, _i, _i, _i, _i, _i, _P(_f), _vp,
                                     _vp, _vp, _vp, _vp, _sz, _vp, _i]),
    'tc_box_decode_kept_path': (_i, [_vp, _vp, _i, _i, _i, _i, _i, _P(_f), _f, _i, _i, _vp, _vp, _vp, _vp, _vp, _i]),
    'tc_head_workspace_bytes': (_sz, [_P(tc_head_weights), _i, _i]),
    'tc_cam_pregather_workspace_bytes': (_sz, [_P(tc_head_weights), _i]),
    'tc_head_packed_bytes': (_sz, [_P(tc_head_weights)]),
    'tc_head_pack_weights': (_i, [_P(tc_head_weights), _vp, _sz,
                                  _P(tc_head_weights), _vp]),
    'tc_head_repack_trainable': (_i, [_P(tc_head_weights), _P(tc_head_weights), _vp]),
    'tc_head_forward': (_i, [_P(tc_head_weights), _P(tc_head_weights),
                             _P(tc_feats_nhwc), _i, _vp,
                             _f, _f, _vp, _i, _i, _vp, _vp, _P(tc_head_aux),
                             _P(tc_head_options), _vp, _sz, _vp]),
    'tc_decoder_heads_packed_bytes': (_sz, [_P(tc_decoder_heads)]),
    'tc_decoder_heads_pack': (_i, [_P(tc_decoder_heads), _vp, _sz, _P(tc_decoder_heads), _vp]),
    'tc_decoder_outputs_fwd': (_i, [_P(tc_decoder_heads), _vp, _vp, _vp, _i, _i, _vp, _vp,
                                    _P(tc_head_options), _vp]),
    'tc_decoder_outputs_levels_fwd': (_i, [_P(tc_decoder_heads), _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp,
                                           _P(tc_head_options), _vp]),
    # training (backward of the trainable radar stack + optimizer)
    'tc_linear_gated_fwd': (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    'tc_linear_bwd_data': (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _f,
                                _i, _vp]),
    'tc_linear_bwd_weight': (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _f,
                                  _vp]),
    'tc_add_layernorm_bwd': (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i,
                                  _i, _vp]),
    'tc_radar_reference_l1': (_i, [_vp, _P(_f), _vp, _vp, _i, _vp]),
    'tc_box_add_ref_fwd': (_i, [_vp, _i, _vp, _i, _vp, _i, _vp, _i, _vp]),
    'tc_box_add_ref_bwd': (_i, [_vp, _i, _vp, _i, _vp]),
    'tc_radar_attn_core_fwd': (_i, [_vp, _f, _vp, _vp, _i, _vp, _i, _vp, _i,
                                    _i, _i, _i, _i, _i, _i, _f, _f, _vp, _vp,
                                    _f, C.c_ulonglong, _i, _vp]),
    'tc_radar_attn_core_fwd_n': (_i, [_vp, _f, _vp, _vp, _i, _vp, _i, _vp, _i,
                                      _i, _i, _i, _i, _i, _i, _f, _f, _vp, _vp,
                                      _f, C.c_ulonglong, _i, _i, _vp]),
    'tc_radar_attn_core_bwd_n': (_i, [_vp, _f, _vp, _vp, _i, _vp, _i, _vp, _i,
                                      _i, _i, _i, _i, _i, _i, _f, _f, _vp, _vp,
                                      _vp, _vp, _f, C.c_ulonglong, _i, _i, _vp]),
    'tc_dropout': (_i, [_vp, _i, _i, _f, C.c_ulonglong, _i, _vp, _vp]),
    'tc_radar_attn_core_bwd': (_i, [_vp, _f, _vp, _vp, _i, _vp, _i, _vp, _i,
                                    _i, _i, _i, _i, _i, _i, _f, _f, _vp, _vp,
                                    _vp, _vp, _f, C.c_ulonglong, _i, _vp]),
    'tc_radar_train_tape_bytes': (_sz, [_P(tc_head_weights), _i, _i]),
    'tc_radar_train_fwd': (_i, [_P(tc_head_weights), _vp, _vp, _vp, _vp, _i, _i,
                                _i, _vp, _vp, _vp, _sz, _f, C.c_ulonglong, _vp]),
    'tc_radar_train_fwd_fused': (_i, [_P(tc_head_weights), _vp, _vp, _vp, _vp, _i, _i,
                                      _i, _vp, _vp, _vp, _sz, _f, C.c_ulonglong, _vp]),
    'tc_head_repack_trainable_ex': (_i, [_P(tc_head_weights), _P(tc_head_weights), _i, _vp]),
    'tc_radar_train_bwd': (_i, [_P(tc_head_weights), _P(tc_head_weights), _vp,
                                _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _sz,
                                _f, C.c_ulonglong, _vp]),
    'tc_radar_train_bwd_workspace_bytes': (_sz, [_P(tc_head_weights), _i, _i]),
    'tc_radar_train_bwd_fused': (_i, [_P(tc_head_weights), _P(tc_head_weights), _vp,
                                      _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp, _sz,
                                      _f, C.c_ulonglong, _vp, _vp, _vp]),
    'tc_radar_train_bwd_fused_ex': (_i, [_P(tc_head_weights), _P(tc_head_weights), _vp,
                                         _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp, _sz,
                                         _f, C.c_ulonglong, _vp, _vp, _i, _vp]),
    'tc_radar_train_bwd_fused_det': (_i, [_P(tc_head_weights), _P(tc_head_weights), _vp,
                                          _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp, _sz,
                                          _f, C.c_ulonglong, _vp, _vp, _i, _vp, _sz, _vp, _sz, _vp]),
    'tc_radar_train_bwd_weights': (_i, [_P(tc_head_weights), _P(tc_head_weights), _vp, _vp, _i, _i, _vp, _sz, _vp, _sz,
                                        _i, _vp]),
    'tc_radar_train_repack': (_i, [_P(tc_head_weights), _P(tc_head_weights), _vp, _sz, _i, _i, _vp]),
    'tc_dropout_mask': (_i, [_f, C.c_ulonglong, _i, _sz, _vp, _vp]),
    'tc_normalize_bbox': (_i, [_vp, _i, _vp, _vp]),
    'tc_match_cost': (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _f, _f,
                           _f, _f, _f, _vp, _vp]),
    'tc_detr_loss_fwd_bwd': (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _i, _vp,
                                  _vp, _vp, _f, _f, _f, _f, _vp, _vp, _vp, _vp]),
    'tc_detr_loss_fwd_bwd_counts': (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _i, _vp,
                                         _vp, _vp, _f, _f, _f, _f, _vp, _vp, _vp, _vp]),
    'tc_lsa_assign': (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    'tc_lsa_assign_ex': (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    'tc_lsa_workspace_bytes': (_sz, [_i, _i, _i, _i]),
    'tc_lsa_assign_ws': (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _sz, _i, _vp]),
    'tc_sq_norm': (_i, [_vp, _sz, _vp, _vp]),
    'tc_adamw_step': (_i, [_vp, _vp, _vp, _vp, _sz, _f, _f, _f, _f, _f, _i, _f,
                           _f, _vp, _vp]),
}

_lib = None


def lib():
    """The loaded library (cached).  Fails loudly when it is not built."""
    global _lib
    if _lib is None:
        if not os.path.isfile(LIB_PATH):
            raise TransCARHipError(
                'HIP library not built: %s is missing.  transcar_amd has no '
                'CPU fallback; run __graft_entry__.build() or '
                '`make -C transcar_amd/csrc`.' % LIB_PATH)
        dll = C.CDLL(LIB_PATH)
        if (hasattr(dll, 'tc_debug_chain_stamps') or hasattr(dll, 'tc_debug_diag_build')) and os.environ.get('TRANSCAR_ALLOW_STAMPS') != '1':
            raise TransCARHipError(
                '%s is the STAMPS debug build (timing switches with wrong results); set '
                'TRANSCAR_ALLOW_STAMPS=1 to use it for tools/chain_stamps.py' % LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(dll, name)        # AttributeError if a symbol is gone
            fn.restype = res
            fn.argtypes = args
        if dll.tc_abi_version() != TC_ABI_VERSION:
            raise TransCARHipError('ABI mismatch: library %d, binding %d' % (
                dll.tc_abi_version(), TC_ABI_VERSION))
        _lib = dll
    return _lib


def check(rc, what):
    if rc != 0:
        msg = lib().tc_last_error().decode('utf-8', 'replace')
        raise TransCARHipError('%s failed (status %d): %s' % (what, rc, msg))


def stream_ptr(device=None):
    """The current HIP stream of `device` (None: of the current device) as the void* every tc_* entry takes last."""
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def size_query(query, *args):
    """A tc_*_bytes query of the library; 0 is its refusal and raises with its message."""
    nbytes = query(*args)
    if nbytes == 0:
        raise TransCARHipError(lib().tc_last_error().decode())
    return nbytes


def device_bytes(device, query, *args):
    """A new byte buffer on `device` of the size ``query(*args)`` asks for (`size_query`)."""
    return torch.empty(size_query(query, *args), dtype=torch.uint8, device=device)


def chain_tile_rows(rows, tile_rows=0, matrix_path=TC_MATRIX_AUTO):
    """The tile height the row chains use for `rows` rows per launch (tc_chain_tile_rows: the library's one rule)."""
    r = lib().tc_chain_tile_rows(int(rows), int(tile_rows), int(matrix_path))
    if r < 0:
        check(r, 'tc_chain_tile_rows')
    return r


def f6(values):
    return (C.c_float * 6)(*[float(v) for v in values])
