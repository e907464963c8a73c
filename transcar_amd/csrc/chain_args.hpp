// Host only: the facts the entry points of head.hip and train_stack.hip share about a head, and one builder per
// launch-argument struct of the radar side (kernels.hpp).  Each returns its struct by value; a caller adds what only it has.
#pragma once
#include <math.h>

#include "kernels.hpp"

namespace tc {

// the K | V half of a fusion layer's in_proj ([3C, C] weight, [3C] bias); a layer a shallow head lacks gives a null pair
inline tc_linear kv_half(const tc_mha& m, int C) {
  return tc_linear{m.in_proj.w ? m.in_proj.w + (size_t)C * C : nullptr, m.in_proj.b ? m.in_proj.b + C : nullptr};
}
// 1 / sqrt(head dimension) of the fusion attention at H heads
inline float radar_qscale(int C, int H) { return 1.0f / sqrtf((float)(C / H)); }
// both halves of tc_head_weights.num_heads, as every entry that takes the struct checks them (`what`: the message's prefix)
inline int check_head_counts(const tc_head_weights* w, const char* what) {
  TC_REQUIRE(w->embed_dims == 256 && heads_ok(decoder_heads(w)), "%sembed_dims=%d num_heads=%d (256 with 4, 8 or 16 heads supported)",
             what, w->embed_dims, decoder_heads(w));
  TC_REQUIRE(heads_ok(radar_heads(w)), "%sradar_num_heads=%d (the upper 16 bits of num_heads: 0, 4, 8 or 16 supported)", what,
             radar_heads(w));
  TC_REQUIRE(w->num_cams >= 1 && w->num_cams <= TC_MAX_CAMS, "%snum_cams=%d (1 .. %d supported)", what, w->num_cams, TC_MAX_CAMS);
  return 0;
}
// The radar input of a head: tokens the reference would attend over (its padded count, the stride of the attention-probability
// dropout's index; 0 reads as TC_RADAR_TOKENS_REF, as a zeroed radar head count reads as TC_RADAR_HEADS) and features per token.
inline int radar_tokens_ref(const tc_head_weights* w) { return w->num_radar_tokens_ref != 0 ? w->num_radar_tokens_ref : TC_RADAR_TOKENS_REF; }
inline int check_radar_input(const tc_head_weights* w, const char* what) {
  TC_REQUIRE(w->num_radar_layers <= 0 || (radar_tokens_ref(w) >= TC_MIN_RADAR_TOKENS && radar_tokens_ref(w) <= TC_MAX_RADAR_TOKENS),
             "%snum_radar_tokens_ref=%d (%d .. %d supported; 0: %d)", what, w->num_radar_tokens_ref, TC_MIN_RADAR_TOKENS,
             TC_MAX_RADAR_TOKENS, TC_RADAR_TOKENS_REF);
  // (a camera-only head reads no token: its feature count only keeps the alignment every caller so far was held to)
  TC_REQUIRE((w->radar_in_dims & 3) == 0 && (w->num_radar_layers <= 0 || (w->radar_in_dims >= 4 && w->radar_in_dims <= TC_MAX_RADAR_IN_DIMS)),
             "%sradar_in_dims=%d (4, 8, .. %d supported)", what, w->radar_in_dims, TC_MAX_RADAR_IN_DIMS);
  return 0;
}
// the forward, training and backward entries: the launch's T against the head's token count ...
inline int check_radar_tokens(const tc_head_weights* w, int T, const char* what) {
  TC_REQUIRE(w->num_radar_layers <= 0 || T <= radar_tokens_ref(w), "%sT=%d is above num_radar_tokens_ref=%d", what, T,
             radar_tokens_ref(w));
  return 0;
}
// ... and, where the attention probabilities are dropped out (dropout_p > 0), their index (row * heads + head) * N + token against 32 bits
inline int check_radar_dropout_index(const tc_head_weights* w, int B, float dropout_p, const char* what) {
  if (!(dropout_p > 0.0f)) return 0;            // no mask is drawn: no index
  const unsigned long long n = (unsigned long long)B * w->num_query * radar_heads(w) * radar_tokens_ref(w);
  TC_REQUIRE(n < (1ull << 32), "%srows * heads * num_radar_tokens_ref = %d * %d * %d = %llu does not fit the dropout index (2^32)",
             what, B * w->num_query, radar_heads(w), radar_tokens_ref(w), n);
  return 0;
}
inline void copy_pc(float (&dst)[6], const float* pc) { for (int i = 0; i < 6; ++i) dst[i] = pc[i]; }
// the box fusion layer r refines: the decoder's last box, then the layer below's output (HEAD:615-617)
inline const float* layer_box_prev(int r, const float* last_box, const float* all_bbox_preds, int rows, int code) {
  return r == 0 ? last_box : all_bbox_preds + (size_t)(r - 1) * rows * code;
}

// radar encoders + the K | V projections of every fusion layer into kv[0 .. TC_MAX_RADAR_LAYERS)
inline RadarEncodeArgs radar_encode_args(const tc_head_weights* w, const float* tokens, int rt, float* const* kv,
                                         float* radar_feat = nullptr, int matrix_path = 0, int* range_status = nullptr) {
  RadarEncodeArgs re;
  re.tokens = tokens; re.RI = w->radar_in_dims; re.M = rt;
  re.rpe = w->radar_position_encoder; re.f0 = w->radar_feat0; re.f2 = w->radar_feat2; re.f4 = w->radar_feat4;
  re.nlayers = w->num_radar_layers;
  for (int r = 0; r < TC_MAX_RADAR_LAYERS; ++r) { re.kvproj[r] = kv_half(w->radar[r].attn, w->embed_dims); re.kv[r] = kv[r]; }
  re.radar_feat = radar_feat; re.w16_delta = w->packed16_delta; re.matrix_path = matrix_path; re.range_status = range_status;
  return re;
}

// fusion layers first_layer .. first_layer + num_layers - 1 on B frames of Q queries and T tokens: kv the K | V of ALL the
// head's layers, all_cls / all_box the [layers, rows, .] outputs of all of them; opt (may be null: the defaults) gives the
// tile height, the matrix path, last_level_cls_only and range_status
inline RadarChainArgs radar_chain_args(const tc_head_weights* w, int first_layer, int num_layers, float* const* kv,
                                       const float* qf, const float* ref_last, const float* box_m, const float* tokens,
                                       int B, int T, int pad_mult, float* all_cls, float* all_box, int* hits,
                                       const tc_head_options* opt = nullptr) {
  const int rows = B * w->num_query;
  RadarChainArgs rc;
  rc.qf = qf; rc.ref_last = ref_last; rc.box_m = box_m; rc.tokens = tokens; rc.RI = w->radar_in_dims;
  for (int r = 0; first_layer + r < TC_MAX_RADAR_LAYERS; ++r) { rc.kv[r] = kv[first_layer + r]; rc.w[r] = w->radar[first_layer + r]; }
  rc.nlayers = num_layers; rc.Q = w->num_query; rc.T = T; rc.pad_mult = pad_mult; rc.code = w->code_size;
  rc.ncls = w->num_classes; rc.M = rows; rc.heads = radar_heads(w); rc.qscale = radar_qscale(w->embed_dims, rc.heads);
  copy_pc(rc.pc, w->pc_range);
  rc.all_cls = all_cls + (size_t)first_layer * rows * w->num_classes;
  rc.all_box = all_box + (size_t)first_layer * rows * w->code_size;
  rc.hits = hits; rc.cen_from_box = first_layer > 0;
  if (opt != nullptr) {
    rc.tile_rows = opt->chain_tile_rows; rc.last_cls_only = opt->last_level_cls_only; rc.matrix_path = opt->matrix_path;
    rc.range_status = opt->range_status;
  }
  return rc;
}

// the gated attention core of one fusion layer (radar_attn.hip); qscale 1: qproj comes scaled
inline RadarAttnArgs radar_attn_args(const float* qproj, const float* kv, const float* centre_xy, int ld_c, const float* box,
                                     int code, const float* radar_xy, int ld_xy, int B, int Q, int T, int C, int H,
                                     int pad_mult, float rmin, float rmax, float* attn_out, int* hit_counts,
                                     float qscale = 1.0f) {
  RadarAttnArgs r;
  r.qproj = qproj; r.ldq = C; r.kv = kv; r.ldkv = 2 * C; r.centre_xy = centre_xy; r.ld_c = ld_c;
  r.box = box; r.code = code; r.radar_xy = radar_xy; r.ld_xy = ld_xy;
  r.B = B; r.Q = Q; r.T = T; r.C = C; r.H = H; r.pad_mult = pad_mult;
  r.rmin = rmin; r.rmax = rmax; r.attn_out = attn_out; r.hit_counts = hit_counts; r.qscale = qscale;
  return r;
}
// ... of fusion layer r of a head: layer 0 gates around cxy (launch_radar_ref_l1), the others around the box they refine
inline RadarAttnArgs radar_attn_args(const tc_head_weights* w, int r, const float* qproj, const float* kv, const float* cxy,
                                     const float* box_prev, const float* tokens, int B, int T, int pad_mult, float* attn_out,
                                     int* hit_counts, float qscale = 1.0f) {
  return radar_attn_args(qproj, kv, r == 0 ? cxy : box_prev, r == 0 ? 2 : w->code_size, box_prev, w->code_size, tokens,
                         w->radar_in_dims, B, w->num_query, T, w->embed_dims, radar_heads(w), pad_mult, w->radar[r].radius_min,
                         w->radar[r].radius_max, attn_out, hit_counts, qscale);
}

}  // namespace tc
