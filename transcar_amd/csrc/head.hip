// C ABI (include/transcar_hip.h) and the launch sequence of the whole hot path:
// Detr3DHead.forward of the reference (HEAD:248-740) in eval mode = 6 decoder
// layers (self-attn, camera cross-attn, FFN, box refinement) + radar encoders +
// 3 distance-gated radar fusion layers.  Every function only enqueues kernels
// on the caller's stream; all scratch comes from the caller's workspace, so a
// forward is capturable into a hipGraph and replayable.
#include <math.h>
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>

#include "chain_args.hpp"

namespace tc {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: %s", what, hipGetErrorString(e));
    return (int)e;
  }
  return 0;
}

int linear(const float* x, int ldx, const tc_linear& w, int M, int K, int N, int act, float* y, int ldy, hipStream_t s,
           const float* x2, const float* res, int ldr, const int* rowgate) {
  GemmArgs g;
  g.X = x; g.ldx = ldx; g.X2 = x2; g.x2_cols = x2 ? ((N + 15) / 16) * 16 : 0;
  g.W = w.w; g.ldw = K; g.bias = w.b; g.R = res; g.ldr = ldr; g.rowgate = rowgate;
  g.Y = y; g.ldy = ldy; g.M = M; g.K = K; g.N = N; g.act = act;
  return launch_gemm(g, s);
}

int layernorm(const float* a, const tc_lnorm& n, float* y, int M, int relu, hipStream_t s, const float* b) {
  LnArgs l;
  l.a = a; l.b = b; l.gamma = n.g; l.beta = n.b; l.y = y; l.M = M; l.relu = relu;
  return launch_ln256(l, s);
}

// q * log2(e)/sqrt(head_dim): the decoder's attention cores exponentiate with 2^x
static float decoder_qscale(int C, int H) { return 1.4426950408889634f / sqrtf((float)(C / H)); }

// mmcv MultiheadAttention wrapper for decoder self-attention:
// out = x + out_proj(MHA(q = k = x + pos, v = x))
static int self_attn(const tc_mha& w, const float* x, const float* pos, float* out, int B, int Q,
                     int C, int H, float* qk, float* vt, int qpad, float* attn_o, hipStream_t s) {
  const int rows = B * Q;
  GemmArgs g;
  g.X = x; g.ldx = C; g.X2 = pos; g.x2_cols = 2 * C;
  g.W = w.in_proj.w; g.ldw = C; g.bias = w.in_proj.b;
  g.Y = qk; g.ldy = 2 * C;
  g.Yt = vt; g.t_col0 = 2 * C; g.t_ld = qpad; g.t_rows_per_batch = Q;
  g.M = rows; g.K = C; g.N = 3 * C;
  g.scale = decoder_qscale(C, H); g.scale_cols = C;
  TC_TRY(launch_gemm(g, s));
  TC_TRY(launch_self_attn_core(qk, qk + C, 2 * C, vt, qpad, attn_o, C, B, Q, H, C / H, s));
  return linear(attn_o, C, w.out_proj, rows, C, C, 0, out, C, s, nullptr, x, C);
}

// Detr3DCrossAtten.num_points of a head (0 in a struct that does not set it: 1)
static int head_points(const tc_head_weights* w) { return w->num_points > 0 ? w->num_points : 1; }

// the camera sampling of B frames of Q queries, by explicit dimensions (pc null: the range stays zero) ...
static CamSampleArgs cam_args(const tc_feats_nhwc& feats, int B, int Q, int C, int num_cams, int num_points,
                              const float* lidar2img, const float* ref, const float* pc, float img_h, float img_w,
                              unsigned long long* pair_counter = nullptr, const float* logits = nullptr,
                              float* out = nullptr, unsigned char* vis = nullptr) {
  CamSampleArgs c;
  c.feats = feats; c.B = B; c.Q = Q; c.C = C; c.num_cams = num_cams; c.num_points = num_points;
  c.lidar2img = lidar2img; c.ref = ref; c.logits = logits;
  if (pc != nullptr) copy_pc(c.pc, pc);
  c.img_h = img_h; c.img_w = img_w; c.out = out; c.vis = vis; c.pair_counter = pair_counter;
  return c;
}
// ... and by a head's, as the decoder chains take it (they sample from their own logits into their own rows)
static CamSampleArgs cam_args(const tc_head_weights* w, const tc_feats_nhwc& feats, int B, const float* lidar2img,
                              const float* ref, float img_h, float img_w, unsigned long long* pair_counter) {
  return cam_args(feats, B, w->num_query, w->embed_dims, w->num_cams, head_points(w), lidar2img, ref, w->pc_range, img_h,
                  img_w, pair_counter);
}

// one decoder layer's chain on the rows of `cam` (ref_in = cam.ref); the caller adds what only some launches have
// (row modulos, box_m, dropout, tile options, the pre-gather, layer 0's constants)
static DecoderChainArgs decoder_layer_args(const tc_decoder_layer* layer, const tc_linear* next_in_proj,
                                           const CamSampleArgs& cam, int code, float qscale, const float* attn_o,
                                           const float* x_in, int x_ld, const float* qe, float* hs, float* ref_out,
                                           float* qk, float* vt, int qpad) {
  DecoderChainArgs d;
  d.attn_o = attn_o; d.x_in = x_in; d.x_ld = x_ld; d.qe = qe; d.Q = cam.Q;
  d.ref_in = cam.ref; d.ref_out = ref_out; d.w = layer; d.next_in_proj = next_in_proj; d.qscale = qscale;
  d.hs = hs; d.qk = qk; d.vt = vt; d.qpad = qpad; d.cam = cam; d.code = code; d.M = cam.B * cam.Q;
  return d;
}

struct CrossWs { float *logits, *sampled, *t0, *pe0, *pe1; };

// Detr3DCrossAtten.forward; returns the pieces the caller fuses with the next
// LayerNorm: t0 = output_proj(sampled) + query, pe1 = position_encoder.3(...)
static int cross_atten_parts(const tc_linear& aw, const tc_linear& oproj, const tc_pos_encoder& pe,
                             const tc_feats_nhwc* feats, int B, int Q, int C, int ncams,
                             const float* query, const float* pos, const float* l2i,
                             const float* ref, const float* pc, float img_h, float img_w,
                             const CrossWs& ws, unsigned long long* pair_counter, hipStream_t s,
                             int np = 1) {
  const int rows = B * Q;
  const int NL = ncams * feats->num_levels * np;       // attention_weights: N * P * L columns (XFMR:362-363)
  TC_TRY(linear(query, C, aw, rows, C, NL, 0, ws.logits, NL, s, pos));
  TC_TRY(launch_cam_sample(cam_args(*feats, B, Q, C, ncams, np, l2i, ref, pc, img_h, img_w, pair_counter, ws.logits, ws.sampled), s));
  TC_TRY(linear(ws.sampled, C, oproj, rows, C, C, 0, ws.t0, C, s, nullptr, query, C));
  TC_TRY(launch_posenc_l1(ref, 3, 1, pe.l0.w, pe.l0.b, pe.n1.g, pe.n1.b, ws.pe0, rows, s));
  return linear(ws.pe0, C, pe.l3, rows, C, C, 0, ws.pe1, C, s);
}

static int check_dims(const tc_head_weights* w) {
  TC_REQUIRE(w != nullptr, "weights pointer is null");
  TC_REQUIRE(w->abi_version == TC_ABI_VERSION, "tc_head_weights.abi_version=%d, library=%d",
             w->abi_version, TC_ABI_VERSION);
  TC_TRY(check_head_counts(w, ""));
  TC_REQUIRE(w->num_layers >= 1 && w->num_layers <= TC_MAX_LAYERS, "num_layers=%d", w->num_layers);
  TC_REQUIRE(w->num_radar_layers >= 0 && w->num_radar_layers <= TC_MAX_RADAR_LAYERS,
             "num_radar_layers=%d (0 .. %d supported)", w->num_radar_layers, TC_MAX_RADAR_LAYERS);
  TC_REQUIRE(w->num_levels >= 1 && w->num_levels <= TC_MAX_LEVELS, "num_levels=%d (1 .. %d supported)", w->num_levels,
             TC_MAX_LEVELS);
  TC_REQUIRE(w->num_points >= 0 && w->num_cams * w->num_levels * head_points(w) <= TC_MAX_CAM_LOGITS,
             "num_points=%d (num_cams * num_levels * num_points <= %d supported)", w->num_points, TC_MAX_CAM_LOGITS);
  TC_REQUIRE(w->num_classes >= 1 && w->num_classes <= TC_MAX_CLASSES, "num_classes=%d (1 .. %d supported)", w->num_classes,
             TC_MAX_CLASSES);
  TC_REQUIRE((w->ffn_dims & 31) == 0, "ffn_dims=%d (a multiple of 32)", w->ffn_dims);
  TC_TRY(check_radar_input(w, ""));
  for (int r = 0; r < w->num_radar_layers; ++r)
    TC_TRY(check_radar_radii(w->radar[r].radius_min, w->radar[r].radius_max, "radar", r));
  return 0;
}

// The entries that read packed weights (the fused row chains): the decoder FFN runs in chunks of 512 hidden units, the last
// one 256 or 512 wide.  (The operator-by-operator forward on the caller's own struct takes check_dims' multiples of 32.)
static int check_ffn_dims_fused(const tc_head_weights* w) {
  TC_REQUIRE(w->ffn_dims >= TC_FFN_DIMS_MIN && w->ffn_dims <= TC_FFN_DIMS_MAX && w->ffn_dims % TC_FFN_DIMS_STEP == 0,
             "ffn_dims=%d (the fused entries take multiples of %d from %d to %d)", w->ffn_dims, TC_FFN_DIMS_STEP,
             TC_FFN_DIMS_MIN, TC_FFN_DIMS_MAX);
  return 0;
}

// Box refinement (with_box_refine, HEAD:45): a head without it hands the decoder reg_branches=None (XFMR:183-203) --
// layers 0 .. L-2 carry reg.l0.w == NULL, and only the last layer's branch (the head's reg_branches[-1], HEAD:287-293)
// exists.  Mixed NULL / set branches below the last layer are refused.  A one-layer decoder always refines.
static int decoder_refines(const tc_head_weights* w, bool* refine) {
  const int L = w->num_layers;
  const bool r = L < 2 || w->layers[0].reg.l0.w != nullptr;
  for (int l = 1; l + 1 < L; ++l)
    TC_REQUIRE((w->layers[l].reg.l0.w != nullptr) == r,
               "layers[%d].reg is %s but layers[0].reg is %s: below the last layer the reg branches are all set (box "
               "refinement) or all NULL (none)", l, r ? "NULL" : "set", r ? "set" : "NULL");
  TC_REQUIRE(w->layers[L - 1].reg.l0.w != nullptr, "layers[%d].reg is NULL: the last layer's reg branch "
             "(reg_branches[-1]) is required with and without box refinement", L - 1);
  *refine = r;
  return 0;
}

struct HeadWs {
  float *pos, *x, *qk, *vt, *attn_o, *t0, *t1, *t2, *ffn_h, *logits, *sampled;
  float *init_ref, *inter_refs, *hs, *reg_tmp, *box_m;
  float *tp0, *tp1, *f0, *f1, *f2, *radar_feat, *kv, *qproj, *rattn, *cxy, *addref, *qf;
  float* kv3[TC_MAX_RADAR_LAYERS];
  int* hits;
  int *perm, *hitflag;        // row order of the radar chain (launch_radar_compact) + its scratch
  int qpad;
};

static size_t head_ws_layout(const tc_head_weights* w, int B, int T, void* base, size_t cap,
                             HeadWs* out) {
  const int Q = w->num_query, C = w->embed_dims, L = w->num_layers;
  // the hidden activation of the operator-by-operator FFNs: the decoder's and the fusion layers' (rf_linear1, HEAD:131)
  const int F = w->ffn_dims > TC_RADAR_FFN_DIMS ? w->ffn_dims : TC_RADAR_FFN_DIMS;
  const size_t rows = (size_t)B * Q, rt = (size_t)B * T;
  const int qpad = ((Q + 15) / 16) * 16;
  Arena a(base, cap);
  HeadWs h;
  h.qpad = qpad;
  h.pos = a.take<float>(rows * C); h.x = a.take<float>(rows * C);
  h.qk = a.take<float>(rows * 2 * C); h.vt = a.take<float>((size_t)B * C * qpad);
  h.attn_o = a.take<float>(rows * C);
  h.t0 = a.take<float>(rows * C); h.t1 = a.take<float>(rows * C); h.t2 = a.take<float>(rows * C);
  h.ffn_h = a.take<float>(rows * F);
  h.logits = a.take<float>(rows * w->num_cams * w->num_levels * head_points(w));
  h.sampled = a.take<float>(rows * C);
  h.init_ref = a.take<float>(rows * 3); h.inter_refs = a.take<float>((size_t)L * rows * 3);
  h.hs = a.take<float>((size_t)L * rows * C);
  h.reg_tmp = a.take<float>(rows * w->code_size); h.box_m = a.take<float>(rows * w->code_size);
  h.tp0 = a.take<float>(rt * C); h.tp1 = a.take<float>(rt * C);
  h.f0 = a.take<float>(rt * 64); h.f1 = a.take<float>(rt * 128); h.f2 = a.take<float>(rt * C);
  h.radar_feat = a.take<float>(rt * C); h.kv = a.take<float>(rt * 2 * C);
  for (int i = 0; i < TC_MAX_RADAR_LAYERS; ++i) h.kv3[i] = a.take<float>(rt * 2 * C);
  h.qproj = a.take<float>(rows * C); h.rattn = a.take<float>(rows * C);
  h.cxy = a.take<float>(rows * 2); h.addref = a.take<float>(rows * 3);
  h.qf = a.take<float>(rows * C);
  h.hits = a.take<int>((size_t)TC_MAX_RADAR_LAYERS * rows);
  h.perm = a.take<int>(rows); h.hitflag = a.take<int>(rows);
  if (out) *out = h;
  return a.off;
}

// Layer 0's pack-time constants (chain.hip PROG_DECODER_L0_T) exist for the heads that take the one-point, four-level
// kernels; they lie behind l0_attn_out in the packed buffer, over the scratch the layer-0 attention was evaluated from:
// TC_L0_VARIANTS blocks of decoder_l0_const_floats(Q) floats.
static bool l0_foldable(const tc_head_weights* w) {
  return head_points(w) == 1 && w->num_levels == TC_MAX_LEVELS && w->num_cams <= 8;
}
static size_t l0_scratch_bytes(const tc_head_weights* w) {
  const size_t Q = w->num_query, C = w->embed_dims, qpad = ((Q + 15) / 16) * 16;
  const size_t scratch = arena_slice(Q * 2 * C, 4) + arena_slice(C * qpad, 4);       // qk, vt of the layer-0 evaluation
  const size_t consts = l0_foldable(w) ? TC_L0_VARIANTS * decoder_l0_const_floats((int)Q) * sizeof(float) : 0;
  return consts > scratch ? consts : scratch;
}
static const float* l0_consts_of(const tc_head_weights* packed_view, int variant) {
  const size_t Q = packed_view->num_query, C = packed_view->embed_dims;
  return packed_view->l0_attn_out + arena_slice(Q * C, 4) / sizeof(float) + (size_t)variant * decoder_l0_const_floats((int)Q);
}

// ---- fused path: 12 launches per frame (chain.hip) ---------------------------
// The attention core in front of a decoder chain follows the chains' variant (tile_variant): launches that run 16- / 32-row
// tiles on the f16 matrix cores take the staged two-plane core (self_attn.hip, round 4) -- 4- / 8-row launches (one or two
// frames: too few workgroups for a form without split keys) and TC_MATRIX_F32 the fp32 core.  A frame's arithmetic is
// therefore fixed by (chain_tile_rows, matrix_path), not by how many frames share a launch.
// Round 6 (opt-in, tc_head_options.cam_pregather): the staged core's launch also carries the camera gather of THIS layer's
// chain `d` (pre-gather workgroups: the layer's reference points are final since the previous chain).
static int launch_layer_attn_core(const tc_head_weights* w, int B, const tc_head_options& opt, const HeadWs& h, int variant,
                                  DecoderChainArgs& d, hipStream_t s) {
  const int Q = w->num_query, C = w->embed_dims, H = decoder_heads(w), rows = B * Q;
  const DropK* drop = opt.decoder_dropout_p > 0.0f ? &d.drop : nullptr;
  if (variant_mm(variant) != 1)
    return launch_self_attn_core(h.qk, h.qk + C, 2 * C, h.vt, h.qpad, h.attn_o, C, B, Q, H, C / H, s, drop);
  PreGatherArgs pga;
  const bool pre = drop == nullptr && opt.cam_pregather == 1;
  if (pre) {
    // scratch: [rows][num_cams][levels][C] level values (only the visible pairs' 4 KiB are ever touched), [rows] masks
    float* pbuf = static_cast<float*>(opt.cam_pregather_ws);
    int* pmask = reinterpret_cast<int*>(pbuf + (size_t)rows * w->num_cams * w->num_levels * C);
    pga.cam = d.cam; pga.M = rows; pga.ref_mod = d.ref_mod; pga.out = pbuf; pga.mask = pmask;
    d.pre = pbuf; d.premask = pmask;
  }
  return launch_self_attn_core_x(h.qk, h.qk + C, 2 * C, h.vt, h.qpad, h.attn_o, C, B, Q, H, C / H, s, drop, pre ? &pga : nullptr);
}

// Phase 1, the decoder layers of this call (all of them, or options.phase's share).  re: the radar encoders, null without
// a radar part.  folded: layer 0 up to its attention output comes from the packed view.
static int fused_decoder_layers(const tc_head_weights* w, const tc_feats_nhwc* feats, int B, const float* lidar2img,
                                float img_h, float img_w, const RadarEncodeArgs* re, unsigned long long* pairs,
                                const tc_head_options& opt, const HeadWs& h, bool refine, bool folded, hipStream_t s) {
  const int Q = w->num_query, C = w->embed_dims, L = w->num_layers, H = decoder_heads(w), rows = B * Q;
  const float* qe = w->query_embedding;
  // the radar encoders and K/V projections do not depend on the decoder: they ride in the launches of two
  // decoder layers as extra workgroups (chain_dual_kernel): layers 0 and 1 in the one-call forward; the LAST
  // two when the forward comes in two phases (options.phase) -- their K/V feed only the fusion stack, and a
  // caller that still has to build the tokens does so while the device runs the layers before
  const int enc_first = opt.phase != 0 && L > 1 ? L - 2 : 0;
  const int lid_begin = opt.phase == 2 ? enc_first : 0, lid_end = opt.phase == 1 ? enc_first : L;
  // train-mode statistics of the frozen decoder: five dropout sites per layer (sites 16 + 8 l + 0..4)
  const bool ddrop = opt.decoder_dropout_p > 0.0f;
  TC_REQUIRE(!ddrop || (unsigned long long)(opt.dropout_seed_stride ? 1 : B) * H * Q * Q < (1ull << 32),
             "decoder dropout: B*H*Q*Q exceeds 32 bits");
  if (re != nullptr && ddrop && opt.phase != 1) TC_TRY(launch_radar_encode(*re, s));     // no ride in the decoder launches then
  // everything in front of layer 0's camera sampling that reads no frame data is a constant too (out_proj, norm0, pe.3),
  // made by the kernel variant this forward selects (bit-identical to running them here)
  const int variant = tile_variant(rows, opt.chain_tile_rows, opt.matrix_path, "head_forward");
  if (variant < 0) return variant;
  const int l0_variant = folded && l0_foldable(w) ? variant : -1;
  if (!folded && opt.phase != 2) {
    PrologueArgs pa;
    pa.qe = qe; pa.Q = Q; pa.M = rows; pa.refpts = w->reference_points;
    pa.in_proj = w->layers[0].self_attn.in_proj; pa.init_ref = h.init_ref; pa.qk = h.qk; pa.vt = h.vt;
    pa.qpad = h.qpad; pa.qscale = decoder_qscale(C, H); pa.w16_delta = w->packed16_delta;
    TC_TRY(launch_prologue(pa, s));
  }
  for (int lid = lid_begin; lid < lid_end; ++lid) {
    const bool l0c = folded && lid == 0;
    // without box refinement every layer samples at the initial reference points (the folded one when layer 0 is) ...
    const bool init_in = lid == 0 || !refine;
    const float* ref_in = init_in ? (folded ? w->l0_init_reference : h.init_ref)
                                  : h.inter_refs + (size_t)(lid - 1) * rows * 3;
    // ... and only the last layer has a reg branch (its box); the point it refines is not used (h.addref: the
    // operator-by-operator path's scratch), every level's reference is filled after the layers
    float* ref_out = refine ? h.inter_refs + (size_t)lid * rows * 3 : h.addref;
    DecoderChainArgs d = decoder_layer_args(
        &w->layers[lid], lid + 1 < L ? &w->layers[lid + 1].self_attn.in_proj : nullptr,
        cam_args(w, *feats, B, lidar2img, ref_in, img_h, img_w, pairs), w->code_size, decoder_qscale(C, H),
        l0c ? w->l0_attn_out : h.attn_o, lid == 0 ? qe + C : h.hs + (size_t)(lid - 1) * rows * C, lid == 0 ? 2 * C : C, qe,
        h.hs + (size_t)lid * rows * C, ref_out, h.qk, h.vt, h.qpad);
    d.attn_mod = l0c ? Q : 0; d.ref_mod = folded && init_in ? Q : 0; d.x_mod = lid == 0 ? Q : 0;
    d.ffn_dims = w->ffn_dims;
    d.box_m = lid == L - 1 ? h.box_m : nullptr;
    if (ddrop) {
      d.drop = make_drop(opt.decoder_dropout_p, opt.dropout_seed, 16u + 8u * (unsigned)lid, 0u);
      if (opt.dropout_seed_stride != 0) { d.drop.seed_stride = opt.dropout_seed_stride; d.drop.rows_per_sample = (unsigned)Q; }
    }
    d.tile_rows = opt.chain_tile_rows; d.matrix_path = opt.matrix_path; d.range_status = opt.range_status;
    if (l0c && l0_variant >= 0) d.l0_consts = l0_consts_of(w, l0_variant);
    if (!l0c) TC_TRY(launch_layer_attn_core(w, B, opt, h, variant, d, s));
    // the radar encoders ride in two launches, half each (all in layer 0 when there is only one layer)
    if (re != nullptr && !ddrop && lid == enc_first) TC_TRY(launch_decoder_chain_with_encoders(d, *re, L > 1 ? 1 : 0, s));
    // (half B is the K/V of fusion layers 1 and 2: a one-layer fusion head has none, its second launch is the plain chain)
    else if (re != nullptr && !ddrop && L > 1 && lid == enc_first + 1 && w->num_radar_layers > 1)
      TC_TRY(launch_decoder_chain_with_encoders(d, *re, 2, s));
    else TC_TRY(launch_decoder_chain(d, s));
  }
  return 0;
}

// Phase 2, the references behind the last decoder layer: what the radar part reads and what the caller asked for
static int fused_references(const tc_head_weights* w, int B, const tc_head_aux* aux, const HeadWs& h, bool refine,
                            bool folded, hipStream_t s) {
  const int Q = w->num_query, rows = B * Q;
  if (!refine)   // inter_references[l] = init_reference (XFMR:183-203 with reg_branches=None): what the radar part reads
    TC_TRY(launch_ref_broadcast(folded ? w->l0_init_reference : h.init_ref, folded ? Q : 0, h.inter_refs, rows, w->num_layers, s));
  if (aux == nullptr || aux->init_reference == nullptr) return 0;
  if (!folded) {
    TC_HIP(hipMemcpyAsync(aux->init_reference, h.init_ref, (size_t)rows * 3 * 4, hipMemcpyDeviceToDevice, s));
    return 0;
  }
  for (int b = 0; b < B; ++b)
    TC_HIP(hipMemcpyAsync(aux->init_reference + (size_t)b * Q * 3, w->l0_init_reference, (size_t)Q * 3 * 4,
                          hipMemcpyDeviceToDevice, s));
  return 0;
}

// Phase 3, the fusion layers of `rc` on the B frames, then their hit counts into hit_counts (may be null).  The one place
// that decides the row order: queries with a radar return inside their first gate go first (the other tiles skip the gated
// part) when asked (radar_row_order 2) or, left to the library (0), with more than 1024 rows.
static int launch_fusion_chain(RadarChainArgs rc, int B, const tc_head_options& opt, const HeadWs& h, int* hit_counts,
                               hipStream_t s) {
  if (opt.radar_row_order == 2 || (opt.radar_row_order == 0 && rc.M > 1024)) {
    TC_TRY(launch_radar_compact(rc.ref_last, rc.box_m, rc.code, rc.cen_from_box, rc.pc, rc.tokens, rc.RI, B, rc.Q, rc.T,
                                rc.w[0].radius_min, rc.w[0].radius_max, h.hitflag, h.perm, s));
    rc.row_perm = h.perm;
  }
  TC_TRY(launch_radar_chain(rc, s));
  if (hit_counts != nullptr)
    TC_HIP(hipMemcpyAsync(hit_counts, h.hits, (size_t)rc.nlayers * rc.M * 4, hipMemcpyDeviceToDevice, s));
  return 0;
}

static int head_forward_fused(const tc_head_weights* w, const tc_feats_nhwc* feats, int B,
                              const float* lidar2img, float img_h, float img_w,
                              const float* radar_tokens, int T, int pad_mult, float* all_cls_scores,
                              float* all_bbox_preds, const tc_head_aux* aux, const tc_head_options& opt,
                              const HeadWs& h_, hipStream_t s) {
  const int C = w->embed_dims, L = w->num_layers, rows = B * w->num_query;
  // the caller's aux tensors ARE the buffers the chains write (and read back for the next layer): no copies
  // at the end of the forward (round 2: four device-to-device copies per forward with aux, e.g. every training
  // iteration)
  HeadWs h = h_;
  if (aux != nullptr) {
    if (aux->inter_states) h.hs = aux->inter_states;
    if (aux->inter_references) h.inter_refs = aux->inter_references;
    if (aux->last_box) h.box_m = aux->last_box;
  }
  const bool radar = w->num_radar_layers > 0;
  bool refine = true;
  TC_TRY(decoder_refines(w, &refine));
  RadarEncodeArgs re;
  if (radar) re = radar_encode_args(w, radar_tokens, B * T, h.kv3, h.radar_feat, opt.matrix_path, opt.range_status);
  // layer 0 up to its attention output is a constant of the checkpoint (pack time) -- in eval
  // mode: with dropout on the attention probabilities it is not
  const bool folded = !(opt.decoder_dropout_p > 0.0f) && w->l0_attn_out != nullptr && w->l0_init_reference != nullptr;
  TC_TRY(fused_decoder_layers(w, feats, B, lidar2img, img_h, img_w, radar ? &re : nullptr, aux ? aux->sample_pairs : nullptr,
                              opt, h, refine, folded, s));
  if (opt.phase == 1) return 0;
  TC_TRY(fused_references(w, B, aux, h, refine, folded, s));
  if (!radar) return 0;
  return launch_fusion_chain(radar_chain_args(w, 0, w->num_radar_layers, h.kv3, h.hs + (size_t)(L - 1) * rows * C,
                                              h.inter_refs + (size_t)(L - 1) * rows * 3, h.box_m, radar_tokens, B, T, pad_mult,
                                              all_cls_scores, all_bbox_preds, h.hits, &opt),
                             B, opt, h, aux ? aux->radar_hit_counts : nullptr, s);
}

// ---- packed weights for the fused chains (pack.hip) --------------------------
struct PackItem { const float* src; int N, K; const float** slot; bool narrow; bool absent; bool chunked; };

static int collect_pack_items(const tc_head_weights* w, tc_head_weights* v, PackItem* it) {
  const int C = w->embed_dims, F = w->ffn_dims, RF = TC_RADAR_FFN_DIMS, NL = w->num_cams * w->num_levels * head_points(w);
  const int code = w->code_size, ncls = w->num_classes;
  int n = 0;
  // narrow: the three 10-column heads the chains evaluate as wave-per-row dot products (K_NARROW): they
  // stay in the nn.Linear layout (the view keeps the caller's pointer: nothing to re-pack after an
  // optimizer step); listed so that the item order / counts stay what tc_head_repack_trainable assumes
  auto add = [&](const tc_linear& src, tc_linear& dst, int N, int K, bool narrow = false, bool absent = false) {
    it[n].src = src.w; it[n].N = N; it[n].K = K; it[n].slot = &dst.w; it[n].narrow = narrow; it[n].absent = absent;
    it[n].chunked = false; ++n;
  };
  add(w->reference_points, v->reference_points, 3, C);
  for (int l = 0; l < w->num_layers; ++l) {
    const tc_decoder_layer& a = w->layers[l]; tc_decoder_layer& b = v->layers[l];
    add(a.self_attn.in_proj, b.self_attn.in_proj, 3 * C, C);
    add(a.self_attn.out_proj, b.self_attn.out_proj, C, C);
    add(a.attention_weights, b.attention_weights, NL, C);
    add(a.output_proj, b.output_proj, C, C);
    add(a.position_encoder.l3, b.position_encoder.l3, C, C);
    add(a.ffn0, b.ffn0, F, C);
    add(a.ffn1, b.ffn1, C, F);
    it[n - 1].chunked = true;
    // a layer without a reg branch (no box refinement, decoder_refines): nothing to pack, the view's slots are NULL
    const bool noreg = a.reg.l0.w == nullptr;
    add(a.reg.l0, b.reg.l0, C, C, false, noreg);
    add(a.reg.l2, b.reg.l2, C, C, false, noreg);
    add(a.reg.l4, b.reg.l4, code, C, true, noreg);
  }
  if (w->num_radar_layers > 0) {
    add(w->radar_position_encoder.l3, v->radar_position_encoder.l3, C, C);
    add(w->radar_feat0, v->radar_feat0, 64, w->radar_in_dims);
    add(w->radar_feat2, v->radar_feat2, 128, 64);
    add(w->radar_feat4, v->radar_feat4, C, 128);
    for (int r = 0; r < w->num_radar_layers; ++r) {
      const tc_radar_layer& a = w->radar[r]; tc_radar_layer& b = v->radar[r];
      add(a.attn.in_proj, b.attn.in_proj, 3 * C, C);
      add(a.attn.out_proj, b.attn.out_proj, C, C);
      add(a.linear1, b.linear1, RF, C);
      add(a.linear2, b.linear2, C, RF);
      add(a.final_cls.l0, b.final_cls.l0, C, C);
      add(a.final_cls.l3, b.final_cls.l3, C, C);
      add(a.final_cls.l6, b.final_cls.l6, ncls, C, true);
      add(a.final_reg.l0, b.final_reg.l0, C, C);
      add(a.final_reg.l2, b.final_reg.l2, C, C);
      add(a.final_reg.l4, b.final_reg.l4, code, C, true);
    }
  }
  return n;
}
constexpr int MAX_PACK_ITEMS = 1 + 10 * TC_MAX_LAYERS + 4 + 10 * TC_MAX_RADAR_LAYERS;

// The re-pack jobs of the trainable weights after an optimizer step, copies = 1 (the 4x4x1 copy) or 3 (+ the 16x16x4 and
// the f16 ones): the same item order as tc_head_pack_weights; the decoder's items (frozen under tools/train.py:245-252)
// and the layer-0 constants keep their packed contents.  For ONE launch (round 2: one launch per weight, 28 launches
// after every optimizer step).  Returns the job count, -1 with the error set (prefixed by `who`).
static int trainable_pack_jobs(const char* who, const tc_head_weights* w, const tc_head_weights* packed_view, int copies,
                               PackJob* jobs) {
  tc_head_weights scratch = *packed_view;
  PackItem items[MAX_PACK_ITEMS];
  const int n = collect_pack_items(w, &scratch, items);
  const size_t delta = packed_view->packed16_delta;
  int nj = 0;
  for (int i = 1 + 10 * w->num_layers; i < n; ++i) {
    TC_REQUIRE(items[i].src != nullptr, "%s: weight %d is null", who, i);
    if (items[i].narrow) continue;                     // read in place by the chains
    // scratch is a copy of the packed view: its slot still holds the packed destination
    float* dst = const_cast<float*>(*items[i].slot);
    jobs[nj] = PackJob{items[i].src, dst, copies == 3 ? dst + delta : nullptr, items[i].N, items[i].K};
    jobs[nj++].PH = copies == 3 ? dst + 2 * delta : nullptr;
  }
  return nj;
}

}  // namespace tc

using namespace tc;

extern "C" {

int tc_abi_version(void) { return TC_ABI_VERSION; }
int tc_chain_tile_rows(int rows, int tile_rows, int matrix_path) {
  const int v = tile_variant(rows, tile_rows, matrix_path, "chain_tile_rows");
  return v < 0 ? v : variant_rows(v);
}
const char* tc_last_error(void) { return g_err; }

int tc_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
  return n;
}

int tc_nchw_to_nhwc(const float* src, float* dst, int n_img, int C, int H, int W, tc_stream_t stream) {
  return launch_nchw_to_nhwc(src, dst, n_img, C, H, W, as_stream(stream));
}

int tc_nchw_to_nhwc_levels(const float* const* src, float* const* dst, int num_levels, int n_img, int C,
                           const int* H, const int* W, tc_stream_t stream) {
  TC_REQUIRE(src != nullptr && dst != nullptr && H != nullptr && W != nullptr, "nchw_to_nhwc_levels: null argument");
  return launch_nchw_to_nhwc_levels(src, dst, num_levels, n_img, C, H, W, as_stream(stream));
}

int tc_radar_build_tokens(const double* raw, const double* times, const int* chan_start, int num_chan,
                          const double* radar_rot, const double* lidar_rot, const double* point_range,
                          float* tokens, int T, int* count, tc_stream_t stream) {
  return launch_radar_ingest(raw, times, chan_start, num_chan, radar_rot, lidar_rot, point_range, tokens, T,
                             TC_RADAR_TOKENS_REF, count, as_stream(stream));
}

int tc_radar_build_tokens_n(const double* raw, const double* times, const int* chan_start, int num_chan,
                            const double* radar_rot, const double* lidar_rot, const double* point_range,
                            float* tokens, int T, int num_tokens, int* count, tc_stream_t stream) {
  TC_TRY(check_radar_budget("radar_build_tokens_n", T, num_tokens));
  return launch_radar_ingest(raw, times, chan_start, num_chan, radar_rot, lidar_rot, point_range, tokens, T,
                             num_tokens, count, as_stream(stream));
}

int tc_radar_build_tokens_batch(const double* raw, const double* times, const tc_radar_frame_desc* desc,
                                int P, int cap, float* tokens, int T, int* count, tc_stream_t stream) {
  return launch_radar_ingest_batch(raw, times, desc, P, cap, tokens, T, TC_RADAR_TOKENS_REF, count, as_stream(stream));
}

int tc_radar_build_tokens_batch_n(const double* raw, const double* times, const tc_radar_frame_desc* desc,
                                  int P, int cap, float* tokens, int T, int num_tokens, int* count, tc_stream_t stream) {
  TC_TRY(check_radar_budget("radar_build_tokens_batch_n", T, num_tokens));
  return launch_radar_ingest_batch(raw, times, desc, P, cap, tokens, T, num_tokens, count, as_stream(stream));
}

int tc_radar_pack_rows_batch(const float* rows, int total_rows, const int* offsets, int P, int radar_in_dims,
                             const double* point_range, float* tokens, int T, int num_tokens, int* count,
                             tc_stream_t stream) {
  return launch_radar_pack_rows(rows, total_rows, offsets, P, radar_in_dims, point_range, tokens, T, num_tokens, count,
                                as_stream(stream));
}

int tc_linear_fwd(const float* x, const float* x2, const float* w, const float* b, const float* res,
                  float* y, int M, int K, int N, int act, tc_stream_t stream) {
  tc_linear lw{w, b};
  return linear(x, K, lw, M, K, N, act, y, N, as_stream(stream), x2, res, N);
}

int tc_add_layernorm_fwd(const float* a, const float* b, const float* gamma, const float* beta,
                         float* y, int M, int C, int relu, tc_stream_t stream) {
  TC_REQUIRE(C == 256, "add_layernorm: C=%d (256 supported)", C);
  LnArgs l;
  l.a = a; l.b = b; l.gamma = gamma; l.beta = beta; l.y = y; l.M = M; l.relu = relu;
  return launch_ln256(l, as_stream(stream));
}

int tc_refine_reference_fwd(const float* reg_out, int code_size, const float* ref, float* new_ref,
                            int M, tc_stream_t stream) {
  TC_REQUIRE(code_size >= 5, "refine_reference: code_size=%d", code_size);
  const float pc0[6] = {0, 0, 0, 1, 1, 1};
  return launch_ref_update(reg_out, code_size, ref, new_ref, nullptr, pc0, M, as_stream(stream));
}

int tc_cam_sample_fuse_fwd(const tc_feats_nhwc* feats, int B, int Q, int C, int num_cams,
                           const float* lidar2img, const float* ref, const float* attn_logits,
                           const float* pc_range, float img_h, float img_w, float* out,
                           unsigned char* vis_mask, unsigned long long* pair_counter,
                           tc_stream_t stream) {
  return tc_cam_sample_fuse_points_fwd(feats, B, Q, C, num_cams, 1, lidar2img, ref, attn_logits, pc_range, img_h, img_w, out,
                                       vis_mask, pair_counter, stream);
}

int tc_cam_sample_fuse_points_fwd(const tc_feats_nhwc* feats, int B, int Q, int C, int num_cams, int num_points,
                                  const float* lidar2img, const float* ref, const float* attn_logits,
                                  const float* pc_range, float img_h, float img_w, float* out,
                                  unsigned char* vis_mask, unsigned long long* pair_counter,
                                  tc_stream_t stream) {
  TC_REQUIRE(feats != nullptr, "feats is null");
  return launch_cam_sample(cam_args(*feats, B, Q, C, num_cams, num_points, lidar2img, ref, pc_range, img_h, img_w, pair_counter,
                                    attn_logits, out, vis_mask), as_stream(stream));
}

size_t tc_cross_atten_points_workspace_bytes(int B, int Q, int C, int num_cams, int num_levels, int num_points) {
  const size_t rows = (size_t)B * Q;
  return arena_slice(rows * num_cams * num_levels * (size_t)(num_points > 0 ? num_points : 1), 4) +
         4 * arena_slice(rows * C, 4);
}

size_t tc_cross_atten_workspace_bytes(int B, int Q, int C, int num_cams, int num_levels) {
  return tc_cross_atten_points_workspace_bytes(B, Q, C, num_cams, num_levels, 1);
}

int tc_cross_atten_points_fwd(const tc_linear* attention_weights, const tc_linear* output_proj,
                              const tc_pos_encoder* position_encoder, const tc_feats_nhwc* feats, int B,
                              int Q, int C, int num_cams, int num_points, const float* query, const float* query_pos,
                              const float* lidar2img, const float* ref, const float* pc_range, float img_h,
                              float img_w, float* out, void* workspace, size_t workspace_bytes,
                              tc_stream_t stream) {
  TC_REQUIRE(C == 256, "cross_atten: C=%d (256 supported)", C);
  TC_REQUIRE(feats != nullptr, "feats is null");
  TC_REQUIRE(feats->num_levels >= 1 && feats->num_levels <= TC_MAX_LEVELS, "cross_atten: num_levels=%d (1 .. %d supported)",
             feats->num_levels, TC_MAX_LEVELS);
  TC_REQUIRE(num_points >= 1 && num_cams * feats->num_levels * num_points <= TC_MAX_CAM_LOGITS,
             "cross_atten: num_points=%d (1 .. %d / (num_cams * num_levels) supported)", num_points, TC_MAX_CAM_LOGITS);
  TC_REQUIRE(workspace_bytes >= tc_cross_atten_points_workspace_bytes(B, Q, C, num_cams, feats->num_levels, num_points),
             "cross_atten: workspace too small");
  const size_t rows = (size_t)B * Q;
  Arena a(workspace, workspace_bytes);
  CrossWs ws;
  ws.logits = a.take<float>(rows * num_cams * feats->num_levels * num_points);
  ws.sampled = a.take<float>(rows * C); ws.t0 = a.take<float>(rows * C);
  ws.pe0 = a.take<float>(rows * C); ws.pe1 = a.take<float>(rows * C);
  hipStream_t s = as_stream(stream);
  TC_TRY(cross_atten_parts(*attention_weights, *output_proj, *position_encoder, feats, B, Q, C,
                           num_cams, query, query_pos, lidar2img, ref, pc_range, img_h, img_w, ws,
                           nullptr, s, num_points));
  // XFMR:378: output + inp_residual + relu(LN(position_encoder.3(.)))
  LnArgs l;
  l.a = ws.t0; l.c = ws.pe1; l.g2 = position_encoder->n4.g; l.b2 = position_encoder->n4.b;
  l.y = out; l.M = (int)rows;
  return launch_ln256(l, s);
}

int tc_cross_atten_fwd(const tc_linear* attention_weights, const tc_linear* output_proj,
                       const tc_pos_encoder* position_encoder, const tc_feats_nhwc* feats, int B,
                       int Q, int C, int num_cams, const float* query, const float* query_pos,
                       const float* lidar2img, const float* ref, const float* pc_range, float img_h,
                       float img_w, float* out, void* workspace, size_t workspace_bytes,
                       tc_stream_t stream) {
  return tc_cross_atten_points_fwd(attention_weights, output_proj, position_encoder, feats, B, Q, C, num_cams, 1,
                                   query, query_pos, lidar2img, ref, pc_range, img_h, img_w, out, workspace,
                                   workspace_bytes, stream);
}

size_t tc_self_attn_workspace_bytes(int B, int Q, int C) {
  const size_t rows = (size_t)B * Q;
  const size_t qpad = ((Q + 15) / 16) * 16;
  return arena_slice(rows * 2 * C, 4) + arena_slice((size_t)B * C * qpad, 4) + arena_slice(rows * C, 4);
}

int tc_self_attn_fwd(const tc_mha* w, const float* x, const float* pos, float* out, int B, int Q,
                     int C, int num_heads, void* workspace, size_t workspace_bytes,
                     tc_stream_t stream) {
  TC_REQUIRE(C == 256 && heads_ok(num_heads), "self_attn: C=%d num_heads=%d (256 with 4, 8 or 16 heads supported)", C, num_heads);
  TC_REQUIRE(workspace_bytes >= tc_self_attn_workspace_bytes(B, Q, C), "self_attn: workspace too small");
  const size_t rows = (size_t)B * Q;
  const int qpad = ((Q + 15) / 16) * 16;
  Arena a(workspace, workspace_bytes);
  float* qk = a.take<float>(rows * 2 * C);
  float* vt = a.take<float>((size_t)B * C * qpad);
  float* ao = a.take<float>(rows * C);
  return self_attn(*w, x, pos, out, B, Q, C, num_heads, qk, vt, qpad, ao, as_stream(stream));
}

int tc_decoder_layer_tail_fwd(const tc_decoder_layer* layer, const tc_linear* next_in_proj,
                              const tc_feats_nhwc* feats, int B, int Q, int num_cams,
                              int code_size, const float* attn_o, const float* x_in,
                              const float* query_embedding, const float* lidar2img,
                              const float* ref_in, const float* pc_range, float img_h,
                              float img_w, float* hs, float* ref_out, float* qk, float* vt,
                              int qpad, int tile_rows, tc_stream_t stream) {
  return tc_decoder_layer_tail_fwd_ffn(layer, next_in_proj, feats, B, Q, num_cams, code_size, attn_o, x_in, query_embedding,
                                       lidar2img, ref_in, pc_range, img_h, img_w, hs, ref_out, qk, vt, qpad, tile_rows, 512,
                                       stream);
}

int tc_decoder_layer_tail_fwd_ffn(const tc_decoder_layer* layer, const tc_linear* next_in_proj,
                                  const tc_feats_nhwc* feats, int B, int Q, int num_cams,
                                  int code_size, const float* attn_o, const float* x_in,
                                  const float* query_embedding, const float* lidar2img,
                                  const float* ref_in, const float* pc_range, float img_h,
                                  float img_w, float* hs, float* ref_out, float* qk, float* vt,
                                  int qpad, int tile_rows, int ffn_dims, tc_stream_t stream) {
  TC_REQUIRE(layer != nullptr && feats != nullptr, "decoder_layer_tail: null argument");
  TC_REQUIRE(feats->num_levels == 4, "decoder_layer_tail: num_levels=%d (4 supported; heads with fewer levels run "
             "through tc_head_forward)", feats->num_levels);
  const int C = 256, H = 8;            // (the layer of the default head: one sampling point, head dimension 32)
  DecoderChainArgs d = decoder_layer_args(layer, next_in_proj, cam_args(*feats, B, Q, C, num_cams, 1, lidar2img, ref_in, pc_range,
                                                                         img_h, img_w), code_size, decoder_qscale(C, H),
                                          attn_o, x_in, C, query_embedding, hs, ref_out, qk, vt, qpad);
  d.tile_rows = TC_TILE_ROWS(tile_rows); d.matrix_path = TC_TILE_MATRIX(tile_rows);
  d.ffn_dims = ffn_dims;               // (launch_decoder_chain refuses a width the chains do not run, naming it)
  TC_REQUIRE(d.matrix_path <= TC_MATRIX_F16X2 && (tile_rows >> 10) == 0, "decoder_layer_tail: tile_rows=0x%x", tile_rows);
  TC_TRY(launch_decoder_chain(d, as_stream(stream)));
  if (layer->reg.l0.w == nullptr)      // no reg branch (a decoder without box refinement): the reference stays
    TC_HIP(hipMemcpyAsync(ref_out, ref_in, (size_t)B * Q * 3 * 4, hipMemcpyDeviceToDevice, as_stream(stream)));
  return 0;
}

int tc_sdpa_fwd(const float* q, const float* k, int ld, const float* vt, int ldt, float* out, int ldo,
                int B, int Q, int num_heads, tc_stream_t stream) {
  return launch_self_attn_core(q, k, ld, vt, ldt, out, ldo, B, Q, num_heads, 32, as_stream(stream));
}

int tc_sdpa_fwd_hd(const float* q, const float* k, int ld, const float* vt, int ldt, float* out, int ldo,
                   int B, int Q, int num_heads, int head_dim, tc_stream_t stream) {
  return launch_self_attn_core(q, k, ld, vt, ldt, out, ldo, B, Q, num_heads, head_dim, as_stream(stream));
}

size_t tc_sdpa_f16x2_workspace_bytes(int, int, int) { return 0; }     // (the staged form needs none)

int tc_sdpa_fwd_f16x2(const float* qk, const float* vt, int ldt, float* out, int ldo, int B, int Q, int num_heads,
                      void* workspace, size_t workspace_bytes, tc_stream_t stream) {
  (void)workspace; (void)workspace_bytes;          // (an earlier form built f16 planes there; the staged form converts in LDS)
  return launch_self_attn_core_x(qk, qk + num_heads * 32, 2 * num_heads * 32, vt, ldt, out, ldo, B, Q, num_heads, 32, as_stream(stream));
}

int tc_sdpa_fwd_f16x2_hd(const float* qk, const float* vt, int ldt, float* out, int ldo, int B, int Q, int num_heads,
                         int head_dim, tc_stream_t stream) {
  TC_REQUIRE(num_heads > 0 && head_dim > 0, "sdpa(f16x2): num_heads=%d head_dim=%d", num_heads, head_dim);
  const int C = num_heads * head_dim;
  return launch_self_attn_core_x(qk, qk + C, 2 * C, vt, ldt, out, ldo, B, Q, num_heads, head_dim, as_stream(stream));
}

size_t tc_radar_xattn_workspace_bytes(int B, int Q, int T, int C) {
  return arena_slice((size_t)B * T * 2 * C, 4) + 2 * arena_slice((size_t)B * Q * C, 4) +
         arena_slice((size_t)B * Q, 4);
}

int tc_radar_gated_xattn_fwd(const tc_mha* w, const float* query, const float* centre_xy,
                             const float* box, int code_size, const float* radar_feat,
                             const float* radar_xy, int B, int Q, int T, int C, int num_heads,
                             int pad_mult, float radius_min, float radius_max, float* out,
                             int* hit_counts, void* workspace, size_t workspace_bytes,
                             tc_stream_t stream) {
  TC_REQUIRE(C == 256 && heads_ok(num_heads), "radar_xattn: C=%d num_heads=%d (256 with 4, 8 or 16 heads supported)", C, num_heads);
  TC_REQUIRE(workspace_bytes >= tc_radar_xattn_workspace_bytes(B, Q, T, C), "radar_xattn: workspace too small");
  TC_TRY(check_radar_radii(radius_min, radius_max, "radar_xattn"));
  hipStream_t s = as_stream(stream);
  const int rows = B * Q, rt = B * T;
  Arena a(workspace, workspace_bytes);
  float* kv = a.take<float>((size_t)rt * 2 * C);
  float* qproj = a.take<float>((size_t)rows * C);
  float* rattn = a.take<float>((size_t)rows * C);
  int* hits = hit_counts ? hit_counts : a.take<int>(rows);
  TC_TRY(linear(radar_feat, C, kv_half(*w, C), rt, C, 2 * C, 0, kv, 2 * C, s));
  GemmArgs g;
  g.X = query; g.ldx = C; g.W = w->in_proj.w; g.ldw = C; g.bias = w->in_proj.b;
  g.Y = qproj; g.ldy = C; g.M = rows; g.K = C; g.N = C;
  g.scale = radar_qscale(C, num_heads); g.scale_cols = C;
  TC_TRY(launch_gemm(g, s));
  TC_TRY(launch_radar_attn(radar_attn_args(qproj, kv, centre_xy, 2, box, code_size, radar_xy, 2, B, Q, T, C, num_heads, pad_mult,
                                           radius_min, radius_max, rattn, hits), s));
  return linear(rattn, C, w->out_proj, rows, C, C, 0, out, C, s, nullptr, query, C, hits);
}

// per-call options of the whole-path entry points (tc_head_forward, tc_radar_fusion_fwd): defaults + validation
static int read_options(const tc_head_options* options, tc_head_options& opt) {
  memset(&opt, 0, sizeof(opt));
  if (options != nullptr) opt = *options;
  TC_REQUIRE(opt.radar_row_order >= 0 && opt.radar_row_order <= 2, "options.radar_row_order=%d (0 automatic, 1 own order, 2 hits first)",
             opt.radar_row_order);
  if (tile_variant(0, opt.chain_tile_rows, opt.matrix_path, "the row chains") < 0) {   // the chains' rule says why
    char why[200];
    snprintf(why, sizeof(why), "%s", g_err);
    TC_REQUIRE(false, "options.chain_tile_rows=%d, options.matrix_path=%d: %s", opt.chain_tile_rows, opt.matrix_path, why);
  }
  TC_REQUIRE(opt.decoder_dropout_p >= 0.0f && opt.decoder_dropout_p < 1.0f, "options.decoder_dropout_p=%g",
             (double)opt.decoder_dropout_p);
  TC_REQUIRE(opt.phase >= 0 && opt.phase <= 2, "options.phase=%d (0 whole forward, 1 before the radar tokens, 2 the rest)",
             opt.phase);
  TC_REQUIRE(opt.phase == 0 || !opt.unfused, "options.phase=%d needs the fused path", opt.phase);
  TC_REQUIRE(opt.cam_pregather == 0 || opt.cam_pregather == 1, "options.cam_pregather=%d (0 off, 1 on)", opt.cam_pregather);
  TC_REQUIRE(opt.cam_pregather == 0 || opt.cam_pregather_ws != nullptr, "options.cam_pregather needs cam_pregather_ws");
  return 0;
}

int tc_radar_fusion_fwd(const tc_head_weights* packed_view, const float* hs_last, const float* ref_last,
                        const float* prev_box, const float* radar_tokens, int B, int T, int pad_mult,
                        int first_layer, int num_layers, float* all_cls_scores, float* all_bbox_preds,
                        int* hit_counts, const tc_head_options* options, void* workspace,
                        size_t workspace_bytes, tc_stream_t stream) {
  const tc_head_weights* w = packed_view;
  TC_TRY(check_dims(w));
  TC_REQUIRE(w->l0_attn_out != nullptr, "radar_fusion: packed_view was not produced by tc_head_pack_weights");
  TC_REQUIRE(first_layer >= 0 && num_layers >= 1 && first_layer + num_layers <= w->num_radar_layers,
             "radar_fusion: layers [%d, %d) of %d", first_layer, first_layer + num_layers, w->num_radar_layers);
  TC_REQUIRE(hs_last && prev_box && radar_tokens && all_cls_scores && all_bbox_preds && (first_layer > 0 || ref_last),
             "radar_fusion: null argument");
  TC_REQUIRE(B >= 1 && T >= 1 && pad_mult >= 1, "radar_fusion: B=%d T=%d pad_mult=%d", B, T, pad_mult);
  TC_TRY(check_radar_tokens(w, T, "radar_fusion: "));
  tc_head_options opt;
  TC_TRY(read_options(options, opt));
  HeadWs h;
  const size_t need = head_ws_layout(w, B, T, workspace, workspace_bytes, &h);
  TC_REQUIRE(need <= workspace_bytes, "workspace too small: need %zu, have %zu", need, workspace_bytes);
  hipStream_t s = as_stream(stream);
  // encoders + K/V projections of all layers (stand-alone encoder program).  As before the builders: this launch gets no
  // range_status (the chain launch below does), so it never raises the sticky non-finite flag
  if (!opt.reuse_radar_kv)
    TC_TRY(launch_radar_encode(radar_encode_args(w, radar_tokens, B * T, h.kv3, h.radar_feat, opt.matrix_path, nullptr), s));
  return launch_fusion_chain(radar_chain_args(w, first_layer, num_layers, h.kv3, hs_last, ref_last, prev_box, radar_tokens, B, T,
                                              pad_mult, all_cls_scores, all_bbox_preds, h.hits, &opt),
                             B, opt, h, hit_counts ? hit_counts + (size_t)first_layer * B * w->num_query : nullptr, s);
}

int tc_radar_gate_selfcheck(int n_radii, unsigned long long seed, unsigned long long* mismatches,
                            tc_stream_t stream) {
  return launch_gate_selfcheck(n_radii, seed, mismatches, as_stream(stream));
}

int tc_radar_gate_selfcheck_range(int n_radii, unsigned long long seed, float rad_lo, float rad_hi, int inclusive,
                                  unsigned long long* mismatches, tc_stream_t stream) {
  return launch_gate_selfcheck_range(n_radii, seed, rad_lo, rad_hi, inclusive, mismatches, as_stream(stream));
}

int tc_rowops_selfcheck(int n_blocks, unsigned long long seed, unsigned long long* mismatches, tc_stream_t stream) {
  return launch_rowops_selfcheck(n_blocks, seed, mismatches, as_stream(stream));
}

size_t tc_box_decode_workspace_bytes(int B, int Q, int num_classes) {
  return box_decode_ws_bytes(B, Q, num_classes);
}

int tc_box_decode_topk(const float* cls_scores, const float* bbox_preds, int B, int Q,
                       int num_classes, int code_size, int max_num, const float* post_center_range,
                       float* boxes, float* scores, int* labels, unsigned char* valid,
                       void* workspace, size_t workspace_bytes, tc_stream_t stream) {
  return launch_box_decode(cls_scores, bbox_preds, B, Q, num_classes, code_size, max_num,
                           post_center_range, boxes, scores, labels, valid, workspace,
                           workspace_bytes, as_stream(stream));
}

int tc_box_decode_kept(const float* cls_scores, const float* bbox_preds, int B, int Q, int num_classes, int code_size,
                       int max_num, const float* post_center_range, float score_threshold, int use_threshold,
                       int z_shift, float* kept_boxes, float* kept_scores, long long* kept_labels, int* kept_count,
                       tc_stream_t stream) {
  BoxDecodeKept k{kept_boxes, kept_scores, kept_labels, kept_count, score_threshold, use_threshold, z_shift};
  return launch_box_decode(cls_scores, bbox_preds, B, Q, num_classes, code_size, max_num, post_center_range,
                           nullptr, nullptr, nullptr, nullptr, nullptr, 0, as_stream(stream), &k);
}

int tc_box_decode_topk_path(const float* cls_scores, const float* bbox_preds, int B, int Q,
                            int num_classes, int code_size, int max_num, const float* post_center_range,
                            float* boxes, float* scores, int* labels, unsigned char* valid,
                            void* workspace, size_t workspace_bytes, tc_stream_t stream, int path) {
  return launch_box_decode(cls_scores, bbox_preds, B, Q, num_classes, code_size, max_num,
                           post_center_range, boxes, scores, labels, valid, workspace,
                           workspace_bytes, as_stream(stream), nullptr, path);
}

int tc_box_decode_kept_path(const float* cls_scores, const float* bbox_preds, int B, int Q, int num_classes, int code_size,
                            int max_num, const float* post_center_range, float score_threshold, int use_threshold,
                            int z_shift, float* kept_boxes, float* kept_scores, long long* kept_labels, int* kept_count,
                            tc_stream_t stream, int path) {
  BoxDecodeKept k{kept_boxes, kept_scores, kept_labels, kept_count, score_threshold, use_threshold, z_shift};
  return launch_box_decode(cls_scores, bbox_preds, B, Q, num_classes, code_size, max_num, post_center_range,
                           nullptr, nullptr, nullptr, nullptr, nullptr, 0, as_stream(stream), &k, path);
}

size_t tc_head_packed_bytes(const tc_head_weights* w) {
  if (check_dims(w) != 0 || check_ffn_dims_fused(w) != 0) return 0;
  bool refine;
  if (decoder_refines(w, &refine) != 0) return 0;
  tc_head_weights view = *w;
  PackItem items[MAX_PACK_ITEMS];
  const int n = collect_pack_items(w, &view, items);
  size_t total = 0;
  for (int i = 0; i < n; ++i)
    if (!items[i].narrow && !items[i].absent) total += 3 * arena_slice(packed_floats(items[i].N, items[i].K), 4);   // + the 16x16x4 and the two-plane f16 copies
  // layer-0 constants + the scratch they are computed from (see tc_head_pack_weights)
  const size_t Q = w->num_query, C = w->embed_dims;
  total += arena_slice(Q * 3, 4) + arena_slice(Q * C, 4) + l0_scratch_bytes(w);
  return total;
}

int tc_head_pack_weights(const tc_head_weights* w, void* packed, size_t packed_bytes,
                         tc_head_weights* packed_view, tc_stream_t stream) {
  TC_TRY(check_dims(w));
  TC_TRY(check_ffn_dims_fused(w));
  bool refine;
  TC_TRY(decoder_refines(w, &refine));
  TC_REQUIRE(packed != nullptr && packed_view != nullptr, "pack_weights: null output");
  TC_REQUIRE(packed_bytes >= tc_head_packed_bytes(w), "pack_weights: buffer too small");
  *packed_view = *w;
  PackItem items[MAX_PACK_ITEMS];
  const int n = collect_pack_items(w, packed_view, items);
  Arena a(packed, packed_bytes);
  // region A: every weight in the 4x4x1 layout; region B: the same weights, same order and slice
  // sizes, in the 16x16x4 layout -- one distance (packed16_delta floats) from any address of a
  // weight (or of a row block of it) to its counterpart; region C: the two-plane f16 copy (4 bytes per weight
  // too), 2 * packed16_delta from region A
  size_t region_a = 0;
  for (int i = 0; i < n; ++i)
    if (!items[i].narrow && !items[i].absent) region_a += arena_slice(packed_floats(items[i].N, items[i].K), 4);
  const size_t delta = region_a / sizeof(float);
  for (int i = 0; i < n; ++i) {
    if (items[i].absent) { *items[i].slot = nullptr; continue; }
    TC_REQUIRE(items[i].src != nullptr, "pack_weights: weight %d is null", i);
    if (items[i].narrow) continue;                     // the view keeps the nn.Linear pointer
    float* dst = a.take<float>(packed_floats(items[i].N, items[i].K));
    // a decoder ffn1 [C, F]: one packed matrix [C, <= 512] per chunk of hidden units the chain runs (chain.hip
    // resolve_program), one behind the other in the weight's slice -- F <= 512 is the one matrix
    const int kc = items[i].chunked ? 512 : items[i].K;
    for (int k0 = 0; k0 < items[i].K; k0 += kc) {
      const int kw = items[i].K - k0 < kc ? items[i].K - k0 : kc;
      float* d = dst + (size_t)items[i].N * k0;
      TC_TRY(launch_pack_linear(items[i].src + k0, items[i].N, kw, items[i].K, d, d + delta, d + 2 * delta, as_stream(stream)));
    }
    *items[i].slot = dst;
  }
  for (int rgn = 0; rgn < 2; ++rgn)
    for (int i = 0; i < n; ++i)
      if (!items[i].narrow && !items[i].absent) a.take<float>(packed_floats(items[i].N, items[i].K));     // regions B, C
  packed_view->packed16_delta = delta;
  for (int l = 0; l < TC_MAX_LAYERS; ++l) packed_view->layers[l].packed16_delta = delta;
  for (int l = 0; l < TC_MAX_RADAR_LAYERS; ++l) packed_view->radar[l].packed16_delta = delta;
  // Layer 0's self-attention input is the learned embedding alone: reference points,
  // QKV projection and softmax(QK^T)V are constants of the checkpoint.  Evaluate them
  // here with the forward's own kernels (prologue chain + attention core, one batch).
  {
    const int Q = w->num_query, C = w->embed_dims, H = decoder_heads(w);
    const int qpad = ((Q + 15) / 16) * 16;
    float* init_ref = a.take<float>((size_t)Q * 3);
    float* attn_o = a.take<float>((size_t)Q * C);
    float* qk = a.take<float>((size_t)Q * 2 * C);
    float* vt = a.take<float>((size_t)C * qpad);
    hipStream_t s = as_stream(stream);
    TC_HIP(hipMemsetAsync(vt, 0, (size_t)C * qpad * 4, s));
    PrologueArgs pa;
    pa.qe = w->query_embedding; pa.Q = Q; pa.M = Q; pa.refpts = packed_view->reference_points;
    pa.in_proj = packed_view->layers[0].self_attn.in_proj; pa.init_ref = init_ref; pa.qk = qk; pa.vt = vt;
    pa.qpad = qpad; pa.qscale = decoder_qscale(C, H);
    pa.w16_delta = delta;
    TC_TRY(launch_prologue(pa, s));
    TC_TRY(launch_self_attn_core(qk, qk + C, 2 * C, vt, qpad, attn_o, C, 1, Q, H, C / H, s));
    packed_view->l0_init_reference = init_ref;
    packed_view->l0_attn_out = attn_o;
    // Layer 0's chain up to the camera sampling, as far as it reads no frame data (out_proj, norm0, pe.3): once per
    // kernel variant a forward can select, by that variant's own kernels (chain.hip PROG_DECODER_L0GEN_T).  The
    // constants overwrite qk / vt, which nothing reads after the attention core above (same stream).
    if (l0_foldable(w)) {
      static_assert(sizeof(float) == 4, "slices are counted in floats");
      tc_feats_nhwc no_feats = {};          // (the camera part is not read: the level count only selects the kernels)
      no_feats.num_levels = w->num_levels;
      DecoderChainArgs d = decoder_layer_args(&packed_view->layers[0], nullptr, cam_args(no_feats, 1, Q, C, w->num_cams, 1, nullptr,
                                                                                          init_ref, nullptr, 0.0f, 0.0f),
                                              w->code_size, pa.qscale, attn_o, w->query_embedding + C, 2 * C, w->query_embedding,
                                              nullptr, nullptr, nullptr, nullptr, qpad);
      d.x_mod = Q; d.ffn_dims = w->ffn_dims;
      for (int v = 0; v < TC_L0_VARIANTS; ++v)
        TC_TRY(launch_decoder_l0_consts(d, v, const_cast<float*>(l0_consts_of(packed_view, v)), s));
    }
  }
  return 0;
}

int tc_head_repack_trainable_ex(const tc_head_weights* w, tc_head_weights* packed_view, int copies,
                                tc_stream_t stream) {
  TC_TRY(check_dims(w));
  TC_REQUIRE(packed_view != nullptr && packed_view->l0_attn_out != nullptr,
             "repack_trainable: packed_view was not produced by tc_head_pack_weights");
  TC_REQUIRE(copies == 1 || copies == 3, "repack_trainable: copies=%d (1: the 4x4x1 copy, 3: both)", copies);
  PackJob jobs[MAX_PACK_ITEMS];
  const int nj = trainable_pack_jobs("repack_trainable", w, packed_view, copies, jobs);
  if (nj <= 0) return nj;
  return launch_pack_group(jobs, nj, as_stream(stream));
}

// train_stack.hip: the pack jobs of the backward's transposed weights (into its workspace)
extern "C" int radar_train_transposed_jobs(const tc_head_weights* w, int B, int T, void* workspace, size_t workspace_bytes,
                                           tc::PackJob* jobs, int cap);

int tc_radar_train_repack(const tc_head_weights* w, tc_head_weights* packed_view, void* bwd_workspace,
                          size_t bwd_workspace_bytes, int B, int T, tc_stream_t stream) {
  TC_TRY(check_dims(w));
  TC_REQUIRE(packed_view != nullptr && packed_view->l0_attn_out != nullptr,
             "radar_train_repack: packed_view was not produced by tc_head_pack_weights");
  PackJob jobs[MAX_PACK_ITEMS + 10 * TC_MAX_RADAR_LAYERS];
  const int nj = trainable_pack_jobs("radar_train_repack", w, packed_view, 1, jobs);
  if (nj < 0) return nj;
  const int nt =radar_train_transposed_jobs(w, B, T, bwd_workspace, bwd_workspace_bytes, jobs + nj, 10 * TC_MAX_RADAR_LAYERS);
  if (nt < 0) return -1;
  return launch_pack_group(jobs, nj + nt, as_stream(stream));
}

int tc_head_repack_trainable(const tc_head_weights* w, tc_head_weights* packed_view,
                             tc_stream_t stream) {
  return tc_head_repack_trainable_ex(w, packed_view, 3, stream);
}

size_t tc_cam_pregather_workspace_bytes(const tc_head_weights* w, int B) {
  if (check_dims(w) != 0 || B < 1) return 0;
  const size_t rows = (size_t)B * w->num_query;
  return rows * ((size_t)w->num_cams * w->num_levels * w->embed_dims * sizeof(float) + sizeof(int));
}

size_t tc_head_workspace_bytes(const tc_head_weights* w, int B, int T) {
  if (check_dims(w) != 0) return 0;
  return head_ws_layout(w, B, T, nullptr, ~size_t(0), nullptr);
}

int tc_head_forward(const tc_head_weights* w, const tc_head_weights* packed_view,
                    const tc_feats_nhwc* feats, int B, const float* lidar2img, float img_h,
                    float img_w, const float* radar_tokens, int T, int pad_mult,
                    float* all_cls_scores, float* all_bbox_preds, const tc_head_aux* aux,
                    const tc_head_options* options, void* workspace, size_t workspace_bytes,
                    tc_stream_t stream) {
  TC_TRY(check_dims(w));
  tc_head_options opt;
  TC_TRY(read_options(options, opt));
  TC_REQUIRE(feats != nullptr, "feats is null");
  TC_REQUIRE(feats->num_levels == w->num_levels, "feats: num_levels=%d, the head's num_levels=%d", feats->num_levels,
             w->num_levels);
  TC_REQUIRE(B >= 1, "B=%d", B);
  TC_REQUIRE(w->num_radar_layers == 0 || (radar_tokens != nullptr && T >= 1 && pad_mult >= 1),
             "radar tokens missing (T=%d pad_mult=%d)", T, pad_mult);
  TC_TRY(check_radar_tokens(w, T, ""));
  HeadWs h;
  const size_t need = head_ws_layout(w, B, T, workspace, workspace_bytes, &h);
  TC_REQUIRE(need <= workspace_bytes, "workspace too small: need %zu, have %zu", need, workspace_bytes);
  TC_REQUIRE(opt.cam_pregather == 0 || w->num_cams <= 8, "options.cam_pregather: num_cams=%d (the camera pre-gather exists for "
             "up to 8 cameras)", w->num_cams);
  TC_REQUIRE(opt.cam_pregather == 0 || opt.cam_pregather_bytes >= tc_cam_pregather_workspace_bytes(w, B),
             "options.cam_pregather_ws holds %zu bytes, %zu needed", opt.cam_pregather_bytes, tc_cam_pregather_workspace_bytes(w, B));
  bool refine = true;
  TC_TRY(decoder_refines(w, &refine));
  hipStream_t s = as_stream(stream);
  const int Q = w->num_query, C = w->embed_dims, F = w->ffn_dims, RF = TC_RADAR_FFN_DIMS, L = w->num_layers, H = decoder_heads(w);
  const int code = w->code_size, ncls = w->num_classes;
  const int rows = B * Q, rt = B * T;
  const float* pc = w->pc_range;
  unsigned long long* pairs = aux ? aux->sample_pairs : nullptr;
  if (packed_view != nullptr && !opt.unfused) TC_TRY(check_ffn_dims_fused(w));
  if (packed_view != nullptr && !opt.unfused)
    return head_forward_fused(packed_view, feats, B, lidar2img, img_h, img_w, radar_tokens, T, pad_mult,
                              all_cls_scores, all_bbox_preds, aux, opt, h, s);
  TC_REQUIRE(opt.decoder_dropout_p == 0.0f && !opt.last_level_cls_only,
             "the operator-by-operator path implements the default options only");

  // ---- operator-by-operator path (options.unfused): the first build, kept
  // as an in-tree cross-check of the fused chains.  XFMR:119-123
  TC_TRY(launch_split_embed(w->query_embedding, Q, C, B, h.pos, h.x, s));
  TC_TRY(launch_init_ref(w->query_embedding, Q, C, w->reference_points.w, w->reference_points.b,
                         h.init_ref, B, s));
  const float* x = h.x;
  for (int lid = 0; lid < L; ++lid) {
    const tc_decoder_layer& ly = w->layers[lid];
    const float* ref_in = lid == 0 || !refine ? h.init_ref : h.inter_refs + (size_t)(lid - 1) * rows * 3;
    float* ref_out = h.inter_refs + (size_t)lid * rows * 3;
    float* hs_l = h.hs + (size_t)lid * rows * C;
    // self_attn, norm
    TC_TRY(self_attn(ly.self_attn, x, h.pos, h.t0, B, Q, C, H, h.qk, h.vt, h.qpad, h.attn_o, s));
    TC_TRY(layernorm(h.t0, ly.norm0, h.t1, rows, 0, s));
    // cross_attn, norm   (XFMR:346-378)
    CrossWs cw{h.logits, h.sampled, h.t0, h.t2, h.attn_o};
    TC_TRY(cross_atten_parts(ly.attention_weights, ly.output_proj, ly.position_encoder, feats, B, Q,
                             C, w->num_cams, h.t1, h.pos, lidar2img, ref_in, pc, img_h, img_w, cw,
                             pairs, s, head_points(w)));
    {
      LnArgs l;
      l.a = h.t0; l.c = h.attn_o; l.g2 = ly.position_encoder.n4.g; l.b2 = ly.position_encoder.n4.b;
      l.gamma = ly.norm1.g; l.beta = ly.norm1.b; l.y = h.t1; l.M = rows;
      TC_TRY(launch_ln256(l, s));
    }
    // ffn, norm
    TC_TRY(linear(h.t1, C, ly.ffn0, rows, C, F, 1, h.ffn_h, F, s));
    TC_TRY(linear(h.ffn_h, F, ly.ffn1, rows, F, C, 0, h.t0, C, s, nullptr, h.t1, C));
    TC_TRY(layernorm(h.t0, ly.norm2, hs_l, rows, 0, s));
    x = hs_l;
    // XFMR:190-203 box refinement of the reference points; without it only the last layer's branch runs, for the box
    if (!refine) {
      TC_HIP(hipMemcpyAsync(ref_out, h.init_ref, (size_t)rows * 3 * 4, hipMemcpyDeviceToDevice, s));
      if (lid != L - 1) continue;
    }
    TC_TRY(linear(hs_l, C, ly.reg.l0, rows, C, C, 1, h.t0, C, s));
    TC_TRY(linear(h.t0, C, ly.reg.l2, rows, C, C, 1, h.t2, C, s));
    TC_TRY(linear(h.t2, C, ly.reg.l4, rows, C, code, 0, h.reg_tmp, code, s));
    TC_TRY(launch_ref_update(h.reg_tmp, code, ref_in, refine ? ref_out : nullptr, lid == L - 1 ? h.box_m : nullptr,
                             pc, rows, s));
  }
  if (aux) {
    if (aux->inter_states)
      TC_HIP(hipMemcpyAsync(aux->inter_states, h.hs, (size_t)L * rows * C * 4, hipMemcpyDeviceToDevice, s));
    if (aux->init_reference)
      TC_HIP(hipMemcpyAsync(aux->init_reference, h.init_ref, (size_t)rows * 3 * 4, hipMemcpyDeviceToDevice, s));
    if (aux->inter_references)
      TC_HIP(hipMemcpyAsync(aux->inter_references, h.inter_refs, (size_t)L * rows * 3 * 4,
                            hipMemcpyDeviceToDevice, s));
    if (aux->last_box)
      TC_HIP(hipMemcpyAsync(aux->last_box, h.box_m, (size_t)rows * code * 4, hipMemcpyDeviceToDevice, s));
  }
  if (w->num_radar_layers == 0) return 0;

  // radar encoders, HEAD:531-536
  const int RI = w->radar_in_dims;
  const tc_pos_encoder& rpe = w->radar_position_encoder;
  TC_TRY(launch_posenc_l1(radar_tokens, RI, 0, rpe.l0.w, rpe.l0.b, rpe.n1.g, rpe.n1.b, h.tp0, rt, s));
  TC_TRY(linear(h.tp0, C, rpe.l3, rt, C, C, 0, h.tp1, C, s));
  TC_TRY(linear(radar_tokens, RI, w->radar_feat0, rt, RI, 64, 1, h.f0, 64, s));
  TC_TRY(linear(h.f0, 64, w->radar_feat2, rt, 64, 128, 1, h.f1, 128, s));
  TC_TRY(linear(h.f1, 128, w->radar_feat4, rt, 128, C, 1, h.f2, C, s));
  {
    LnArgs l;
    l.a = h.tp1; l.gamma = rpe.n4.g; l.beta = rpe.n4.b; l.relu = 1; l.d = h.f2; l.y = h.radar_feat;
    l.M = rt;
    TC_TRY(launch_ln256(l, s));
  }
  // HEAD:543-547, 596-598
  TC_TRY(launch_radar_ref_l1(h.inter_refs + (size_t)(L - 1) * rows * 3, pc, h.cxy, h.addref, rows, s));
  const float* qf = h.hs + (size_t)(L - 1) * rows * C;
  for (int r = 0; r < w->num_radar_layers; ++r) {
    const tc_radar_layer& rl = w->radar[r];
    float* cls_out = all_cls_scores + (size_t)r * rows * ncls;
    float* box_out = all_bbox_preds + (size_t)r * rows * code;
    const float* box_prev = layer_box_prev(r, h.box_m, all_bbox_preds, rows, code);
    int* hits = h.hits + (size_t)r * rows;
    TC_TRY(linear(h.radar_feat, C, kv_half(rl.attn, C), rt, C, 2 * C, 0, h.kv, 2 * C, s));
    GemmArgs g;
    g.X = qf; g.ldx = C; g.W = rl.attn.in_proj.w; g.ldw = C; g.bias = rl.attn.in_proj.b;
    g.Y = h.qproj; g.ldy = C; g.M = rows; g.K = C; g.N = C; g.scale = radar_qscale(C, radar_heads(w)); g.scale_cols = C;
    TC_TRY(launch_gemm(g, s));
    TC_TRY(launch_radar_attn(radar_attn_args(w, r, h.qproj, h.kv, h.cxy, box_prev, radar_tokens, B, T, pad_mult, h.rattn, hits), s));
    // HEAD:581-586
    TC_TRY(linear(h.rattn, C, rl.attn.out_proj, rows, C, C, 0, h.t0, C, s, nullptr, qf, C, hits));
    TC_TRY(layernorm(h.t0, rl.norm2, h.t1, rows, 0, s));
    TC_TRY(linear(h.t1, C, rl.linear1, rows, C, RF, 1, h.ffn_h, RF, s));
    TC_TRY(linear(h.ffn_h, RF, rl.linear2, rows, RF, C, 0, h.t0, C, s, nullptr, h.t1, C));
    TC_TRY(layernorm(h.t0, rl.norm3, h.qf, rows, 0, s));
    qf = h.qf;
    // final_cls / final_reg, HEAD:592-600
    TC_TRY(linear(h.qf, C, rl.final_cls.l0, rows, C, C, 0, h.t0, C, s));
    TC_TRY(layernorm(h.t0, rl.final_cls.n1, h.t2, rows, 1, s));
    TC_TRY(linear(h.t2, C, rl.final_cls.l3, rows, C, C, 0, h.t0, C, s));
    TC_TRY(layernorm(h.t0, rl.final_cls.n4, h.t2, rows, 1, s));
    TC_TRY(linear(h.t2, C, rl.final_cls.l6, rows, C, ncls, 0, cls_out, ncls, s));
    TC_TRY(linear(h.qf, C, rl.final_reg.l0, rows, C, C, 1, h.t0, C, s));
    TC_TRY(linear(h.t0, C, rl.final_reg.l2, rows, C, C, 1, h.t2, C, s));
    TC_TRY(linear(h.t2, C, rl.final_reg.l4, rows, C, code, 0, h.reg_tmp, code, s));
    if (r == 0)
      TC_TRY(launch_box_add_ref(h.reg_tmp, code, h.addref, 3, h.addref + 2, 3, box_out, nullptr, rows, s));
    else
      TC_TRY(launch_box_add_ref(h.reg_tmp, code, box_prev, code, box_prev + 4, code, box_out, nullptr,
                                rows, s));
  }
  if (aux && aux->radar_hit_counts)
    TC_HIP(hipMemcpyAsync(aux->radar_hit_counts, h.hits, (size_t)w->num_radar_layers * rows * 4,
                          hipMemcpyDeviceToDevice, s));
  return 0;
}

// ---- the decoder levels' own class / box branches (chain.hip PROG_DECODER_HEADS) ----
static int check_decoder_heads(const tc_decoder_heads* w, const char* who) {
  TC_REQUIRE(w != nullptr, "%s: null tc_decoder_heads", who);
  TC_REQUIRE(w->abi_version == TC_ABI_VERSION, "%s: tc_decoder_heads.abi_version=%d, the library's is %d", who,
             w->abi_version, TC_ABI_VERSION);
  TC_REQUIRE(w->embed_dims == 256, "%s: embed_dims=%d (256 supported)", who, w->embed_dims);
  TC_REQUIRE(w->num_levels >= 1 && w->num_levels <= TC_MAX_LAYERS, "%s: num_levels=%d (1 .. %d)", who, w->num_levels,
             TC_MAX_LAYERS);
  TC_REQUIRE(w->num_classes >= 1 && w->num_classes <= 32, "%s: num_classes=%d (1 .. 32)", who, w->num_classes);
  TC_REQUIRE(w->code_size >= 8 && w->code_size <= 10, "%s: code_size=%d (8 .. 10)", who, w->code_size);
  for (int l = 0; l < w->num_levels; ++l) {
    const tc_cls_branch& c = w->cls[l]; const tc_reg_branch& g = w->reg[l];
    const void* p[] = {c.l0.w, c.l0.b, c.n1.g, c.n1.b, c.l3.w, c.l3.b, c.n4.g, c.n4.b, c.l6.w, c.l6.b,
                       g.l0.w, g.l0.b, g.l2.w, g.l2.b, g.l4.w, g.l4.b};
    for (size_t i = 0; i < sizeof(p) / sizeof(p[0]); ++i)
      TC_REQUIRE(p[i] != nullptr, "%s: a weight of level %d is null (%s pointer %d)", who, l, i < 10 ? "cls_branches" : "reg_branches",
                 (int)(i < 10 ? i : i - 10));
  }
  return 0;
}

// the four packed matrices of a level and where an earlier level already names the same source
struct HeadsPackSlot { const float* src; const float** slot; };
static int decoder_heads_slots(const tc_decoder_heads* w, tc_decoder_heads* v, HeadsPackSlot* it) {
  int n = 0;
  for (int l = 0; l < w->num_levels; ++l) {
    it[n++] = HeadsPackSlot{w->cls[l].l0.w, &v->cls[l].l0.w};
    it[n++] = HeadsPackSlot{w->cls[l].l3.w, &v->cls[l].l3.w};
    it[n++] = HeadsPackSlot{w->reg[l].l0.w, &v->reg[l].l0.w};
    it[n++] = HeadsPackSlot{w->reg[l].l2.w, &v->reg[l].l2.w};
  }
  return n;
}
static int heads_first_use(const HeadsPackSlot* it, int i) {
  for (int j = 0; j < i; ++j)
    if (it[j].src == it[i].src) return j;
  return i;
}

size_t tc_decoder_heads_packed_bytes(const tc_decoder_heads* w) {
  if (check_decoder_heads(w, "decoder_heads_packed_bytes") != 0) return 0;
  tc_decoder_heads view = *w;
  HeadsPackSlot it[4 * TC_MAX_LAYERS];
  const int n = decoder_heads_slots(w, &view, it);
  size_t total = 0;
  for (int i = 0; i < n; ++i)
    if (heads_first_use(it, i) == i) total += 3 * arena_slice(packed_floats(256, 256), 4);
  return total;
}

int tc_decoder_heads_pack(const tc_decoder_heads* w, void* packed, size_t packed_bytes, tc_decoder_heads* packed_view,
                          tc_stream_t stream) {
  TC_TRY(check_decoder_heads(w, "decoder_heads_pack"));
  TC_REQUIRE(packed != nullptr && packed_view != nullptr, "decoder_heads_pack: null output");
  TC_REQUIRE(packed_bytes >= tc_decoder_heads_packed_bytes(w), "decoder_heads_pack: buffer too small");
  *packed_view = *w;
  HeadsPackSlot it[4 * TC_MAX_LAYERS];
  const int n = decoder_heads_slots(w, packed_view, it);
  // regions as tc_head_pack_weights lays them out: the 4x4x1 copies, then the 16x16x4 copies, then the f16 planes
  size_t distinct = 0;
  for (int i = 0; i < n; ++i) distinct += heads_first_use(it, i) == i;
  const size_t slice = arena_slice(packed_floats(256, 256), 4);
  const size_t delta = distinct * slice / sizeof(float);
  Arena a(packed, packed_bytes);
  for (int i = 0; i < n; ++i) {
    const int first = heads_first_use(it, i);
    if (first != i) { *it[i].slot = *it[first].slot; continue; }     // (a shared branch: packed once)
    float* dst = a.take<float>(packed_floats(256, 256));
    TC_TRY(launch_pack_linear(it[i].src, 256, 256, 256, dst, dst + delta, dst + 2 * delta, as_stream(stream)));
    *it[i].slot = dst;
  }
  packed_view->packed16_delta = delta;
  return 0;
}

int tc_decoder_outputs_levels_fwd(const tc_decoder_heads* packed_view, const float* inter_states, const float* init_reference,
                                  const float* inter_references, int B, int Q, int first_level, int num_levels,
                                  float* cls_out, float* box_out, const tc_head_options* options, tc_stream_t stream) {
  const tc_decoder_heads* w = packed_view;
  TC_TRY(check_decoder_heads(w, "decoder_outputs"));
  TC_REQUIRE(w->packed16_delta != 0, "decoder_outputs: packed_view was not produced by tc_decoder_heads_pack");
  TC_REQUIRE(inter_states && init_reference && cls_out && box_out && (w->num_levels == 1 || inter_references),
             "decoder_outputs: null argument");
  TC_REQUIRE(B >= 1 && Q >= 1, "decoder_outputs: B=%d Q=%d", B, Q);
  TC_REQUIRE(first_level >= 0, "decoder_outputs: first_level=%d (0 .. %d)", first_level, w->num_levels - 1);
  TC_REQUIRE(num_levels >= 1, "decoder_outputs: num_levels=%d (at least one level)", num_levels);
  TC_REQUIRE(first_level <= w->num_levels - num_levels, "decoder_outputs: first_level=%d + num_levels=%d exceeds the %d levels of the view",
             first_level, num_levels, w->num_levels);
  tc_head_options opt;
  TC_TRY(read_options(options, opt));
  TC_REQUIRE(opt.decoder_dropout_p == 0.0f, "decoder_outputs: options.decoder_dropout_p=%g (eval-mode levels only)",
             (double)opt.decoder_dropout_p);
  TC_REQUIRE(!opt.unfused, "decoder_outputs: options.unfused=%d (the decoder heads exist as a row chain only)", opt.unfused);
  DecoderHeadsArgs a;
  a.first = first_level; a.levels = num_levels; a.M = B * Q;
  for (int l = 0; l < num_levels; ++l) { a.cls[l] = w->cls[first_level + l]; a.reg[l] = w->reg[first_level + l]; }
  a.w16_delta = w->packed16_delta;
  a.hs = inter_states; a.init_ref = init_reference; a.inter_refs = inter_references;
  a.all_cls = cls_out; a.all_box = box_out;
  a.ncls = w->num_classes; a.code = w->code_size;
  copy_pc(a.pc, w->pc_range);
  a.tile_rows = opt.chain_tile_rows; a.matrix_path = opt.matrix_path; a.range_status = opt.range_status;
  return launch_decoder_heads(a, as_stream(stream));
}

int tc_decoder_outputs_fwd(const tc_decoder_heads* packed_view, const float* inter_states, const float* init_reference,
                           const float* inter_references, int B, int Q, float* all_cls_scores, float* all_bbox_preds,
                           const tc_head_options* options, tc_stream_t stream) {
  // (a null view is refused by the range entry's own check, before num_levels is read there)
  return tc_decoder_outputs_levels_fwd(packed_view, inter_states, init_reference, inter_references, B, Q, 0,
                                       packed_view != nullptr ? packed_view->num_levels : 1, all_cls_scores, all_bbox_preds,
                                       options, stream);
}

// ---- training entry points (train.hip) ---------------------------------------
int tc_linear_gated_fwd(const float* x, const float* w, const float* b, const float* res,
                        const int* row_gate, float* y, int M, int K, int N, tc_stream_t stream) {
  tc_linear lw{w, b};
  return linear(x, K, lw, M, K, N, 0, y, N, as_stream(stream), nullptr, res, N, row_gate);
}

int tc_linear_bwd_data(const float* dy, const float* y_relu, const int* row_gate, const float* w,
                       const float* x_relu, float* dx, int M, int K, int N, float alpha,
                       int accumulate, tc_stream_t stream) {
  return launch_linear_bwd_data(dy, y_relu, row_gate, w, x_relu, dx, M, K, N, alpha, accumulate,
                                as_stream(stream));
}

int tc_linear_bwd_weight(const float* x, const float* dy, const float* y_relu, const int* row_gate,
                         float* dw, float* db, int M, int K, int N, float alpha,
                         tc_stream_t stream) {
  return launch_linear_bwd_weight(x, dy, y_relu, row_gate, dw, db, M, K, N, alpha, as_stream(stream));
}

int tc_add_layernorm_bwd(const float* a, const float* b, const float* gamma, const float* dy,
                         const float* y_relu, float* dz, float* dgamma, float* dbeta, int M, int C,
                         tc_stream_t stream) {
  TC_REQUIRE(C == 256, "layernorm_bwd: C=%d (256 supported)", C);
  return launch_ln256_bwd(a, b, gamma, dy, y_relu, dz, dgamma, dbeta, M, as_stream(stream));
}

int tc_radar_reference_l1(const float* ref, const float* pc_range, float* centre_xy, float* add_ref,
                          int M, tc_stream_t stream) {
  return launch_radar_ref_l1(ref, pc_range, centre_xy, add_ref, M, as_stream(stream));
}

int tc_box_add_ref_fwd(const float* reg_out, int code_size, const float* ref_xy, int ld_xy,
                       const float* ref_z, int ld_z, float* box, int M, tc_stream_t stream) {
  return launch_box_add_ref(reg_out, code_size, ref_xy, ld_xy, ref_z, ld_z, box, nullptr, M,
                            as_stream(stream));
}

int tc_box_add_ref_bwd(const float* d_box, int code_size, float* d_prev_box, int M,
                       tc_stream_t stream) {
  return launch_box_ref_bwd(d_box, code_size, d_prev_box, M, as_stream(stream));
}

// the attention probabilities' dropout index (row * heads + head) * num_tokens + token of the two core entries
static int check_core_stride(const char* who, int B, int Q, int T, int num_heads, int num_tokens, float dropout_p) {
  TC_TRY(check_radar_budget(who, T, num_tokens));
  const unsigned long long n = (unsigned long long)B * Q * num_heads * num_tokens;
  TC_REQUIRE(dropout_p == 0.0f || n < (1ull << 32), "%s: rows * heads * num_tokens = %d * %d * %d = %llu does not fit the dropout index (2^32)",
             who, B * Q, num_heads, num_tokens, n);
  return 0;
}

int tc_radar_attn_core_fwd(const float* qproj, float q_scale, const float* kv,
                           const float* centre_xy, int ld_c, const float* box, int code_size,
                           const float* radar_xy, int ld_xy, int B, int Q, int T, int C,
                           int num_heads, int pad_mult, float radius_min, float radius_max,
                           float* attn_out, int* hit_counts, float dropout_p,
                           unsigned long long dropout_seed, int dropout_site, tc_stream_t stream) {
  return tc_radar_attn_core_fwd_n(qproj, q_scale, kv, centre_xy, ld_c, box, code_size, radar_xy, ld_xy, B, Q, T, C, num_heads,
                                  pad_mult, radius_min, radius_max, attn_out, hit_counts, dropout_p, dropout_seed, dropout_site,
                                  0, stream);
}

int tc_radar_attn_core_fwd_n(const float* qproj, float q_scale, const float* kv,
                             const float* centre_xy, int ld_c, const float* box, int code_size,
                             const float* radar_xy, int ld_xy, int B, int Q, int T, int C,
                             int num_heads, int pad_mult, float radius_min, float radius_max,
                             float* attn_out, int* hit_counts, float dropout_p,
                             unsigned long long dropout_seed, int dropout_site, int num_tokens, tc_stream_t stream) {
  if (num_tokens != 0) TC_TRY(check_core_stride("radar_attn_core_n", B, Q, T, num_heads, num_tokens, dropout_p));
  const unsigned stride = num_tokens != 0 ? (unsigned)num_tokens : (unsigned)TC_RADAR_TOKENS_REF;
  TC_REQUIRE(C == 256 && heads_ok(num_heads), "radar_attn_core: C=%d num_heads=%d (256 with 4, 8 or 16 heads supported)", C, num_heads);
  TC_REQUIRE(attn_out != nullptr && hit_counts != nullptr, "radar_attn_core: NULL output");
  TC_REQUIRE(dropout_p >= 0.0f && dropout_p < 1.0f, "radar_attn_core: dropout_p=%g", (double)dropout_p);
  TC_TRY(check_radar_radii(radius_min, radius_max, "radar_attn_core"));
  RadarAttnArgs r = radar_attn_args(qproj, kv, centre_xy, ld_c, box, code_size, radar_xy, ld_xy, B, Q, T, C, num_heads, pad_mult,
                                    radius_min, radius_max, attn_out, hit_counts, q_scale);
  r.drop = make_drop(dropout_p, dropout_seed, (unsigned)dropout_site, stride);
  return launch_radar_attn(r, as_stream(stream));
}

int tc_radar_attn_core_bwd(const float* qproj, float q_scale, const float* kv,
                           const float* centre_xy, int ld_c, const float* box, int code_size,
                           const float* radar_xy, int ld_xy, int B, int Q, int T, int C,
                           int num_heads, int pad_mult, float radius_min, float radius_max,
                           const float* attn_out, const float* d_attn, float* dq, float* dkv,
                           float dropout_p, unsigned long long dropout_seed, int dropout_site,
                           tc_stream_t stream) {
  return tc_radar_attn_core_bwd_n(qproj, q_scale, kv, centre_xy, ld_c, box, code_size, radar_xy, ld_xy, B, Q, T, C, num_heads,
                                  pad_mult, radius_min, radius_max, attn_out, d_attn, dq, dkv, dropout_p, dropout_seed,
                                  dropout_site, 0, stream);
}

int tc_radar_attn_core_bwd_n(const float* qproj, float q_scale, const float* kv,
                             const float* centre_xy, int ld_c, const float* box, int code_size,
                             const float* radar_xy, int ld_xy, int B, int Q, int T, int C,
                             int num_heads, int pad_mult, float radius_min, float radius_max,
                             const float* attn_out, const float* d_attn, float* dq, float* dkv,
                             float dropout_p, unsigned long long dropout_seed, int dropout_site,
                             int num_tokens, tc_stream_t stream) {
  if (num_tokens != 0) TC_TRY(check_core_stride("radar_attn_core_bwd_n", B, Q, T, num_heads, num_tokens, dropout_p));
  const unsigned stride = num_tokens != 0 ? (unsigned)num_tokens : (unsigned)TC_RADAR_TOKENS_REF;
  TC_REQUIRE(C == 256 && heads_ok(num_heads), "radar_attn_core_bwd: C=%d num_heads=%d (256 with 4, 8 or 16 heads supported)", C,
             num_heads);
  TC_REQUIRE(dropout_p >= 0.0f && dropout_p < 1.0f, "radar_attn_core_bwd: dropout_p=%g", (double)dropout_p);
  TC_TRY(check_radar_radii(radius_min, radius_max, "radar_attn_core_bwd"));
  RadarAttnArgs r = radar_attn_args(qproj, kv, centre_xy, ld_c, box, code_size, radar_xy, ld_xy, B, Q, T, C, num_heads, pad_mult,
                                    radius_min, radius_max, const_cast<float*>(attn_out), nullptr);     // (q_scale: the launch's)
  r.drop = make_drop(dropout_p, dropout_seed, (unsigned)dropout_site, stride);
  return launch_radar_attn_bwd(r, q_scale, d_attn, dq, dkv, as_stream(stream));
}

int tc_dropout(const float* x, int rows, int cols, float dropout_p, unsigned long long seed, int site,
               float* out, tc_stream_t stream) {
  TC_REQUIRE(dropout_p >= 0.0f && dropout_p < 1.0f, "dropout: p=%g", (double)dropout_p);
  return launch_dropout(x, nullptr, nullptr, rows, cols, make_drop(dropout_p, seed, (unsigned)site, 1500u), out,
                        as_stream(stream));
}

int tc_sq_norm(const float* g, size_t n, float* out, tc_stream_t stream) {
  return launch_sqnorm(g, n, out, as_stream(stream));
}

int tc_adamw_step(float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1,
                  float beta2, float eps, float weight_decay, int step, float grad_scale,
                  float max_norm, const float* sq_norm, tc_stream_t stream) {
  return launch_adamw(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, step, grad_scale, max_norm,
                      sq_norm, as_stream(stream));
}

}  // extern "C"
