// Backward kernels of the trainable part of the head (SURVEY.md section 8 rows
// a16 / e / f3): tools/train.py:245-252 freezes the DETR3D decoder, so one
// training iteration differentiates the radar encoders (HEAD:531-536), the three
// gated radar fusion layers (HEAD:573-590 and the _2/_3 copies) and the
// final_cls*/final_reg* MLPs (HEAD:592-600) -- 2,646,316 parameters.
//
//   bwd_gemm_kernel<DATA>    dX[M,K]  = dY~[M,N] W[N,K]          (nn.Linear, input grad)
//   bwd_gemm_kernel<WEIGHT>  dW[N,K] += dY~^T[N,M] X[M,K],  db[N] += colsum dY~
//        dY~ = dY with the layer's own ReLU mask (its saved output <= 0) and the
//        row gate of the radar out_proj (rows without a radar hit, HEAD:581)
//        applied while the tile is staged, so no masked copy is materialised.
//        f32 MFMA 16x16x4 (exact f32 FMA chain) from LDS tiles; WEIGHT splits the
//        900-row reduction over the grid and meets in fp32 atomics.
//   ln_bwd_kernel            LayerNorm(a (+b)) (+ReLU): dz, dgamma +=, dbeta +=
//   radar_attn_bwd_kernel    the gated attention core: one wavefront per query,
//        the gate is re-evaluated exactly as in the forward (rowdev.hpp cdist_mm),
//        softmax statistics are recomputed over the few hit tokens, dK/dV go to
//        the token rows with atomics.
//   box_ref_bwd_kernel, sqnorm / adamw kernels (flat bucket, device-side clip).
#include "kernels.hpp"
#include "rowdev.hpp"

namespace tc {

#define MFMA4(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

enum { BWD_DATA = 0, BWD_WEIGHT = 1 };

struct BwdGemmK {
  const float* A; const float* relu; const int* gate; const float* Bm;
  const float* cmask;          // DATA: zero dX where cmask (the producer's ReLU output) <= 0
  float* C; float* colsum;
  int ldA, ldB, ldC, I, J, R, rchunk, accumulate;
  float alpha;
};

// C[I,J] (+)= alpha * sum_r A(i,r) B(r,j),  B(r,j) = Bm[r*ldB + j]
//   DATA:   A(i,r) = dY[i*ldA + r]   (i = row m, r = n)
//   WEIGHT: A(i,r) = dY[r*ldA + i]   (i = n,     r = row m)
// Tile 64 x BN, reduction step 32; the next step's operands are fetched into
// registers while the MFMAs of the current one run (the loop is latency-bound:
// these GEMMs are 900 x 256 x 256).  4 waves = 4 row groups of 16, NT = BN/16
// accumulators each.
constexpr int BG_RK = 32;

template <int MODE>
__device__ __forceinline__ float bg_load_a(const BwdGemmK& p, int gi, int gr, int rend) {
  float v = 0.f;
  if (gi < p.I && gr < rend) {
    const size_t off = MODE == BWD_DATA ? (size_t)gi * p.ldA + gr : (size_t)gr * p.ldA + gi;
    v = p.A[off];
    if (p.relu != nullptr && p.relu[off] <= 0.f) v = 0.f;
    if (p.gate != nullptr && p.gate[MODE == BWD_DATA ? gi : gr] <= 0) v = 0.f;
  }
  return v;
}

// VEC: 16-byte global loads of the operand tiles (every leading dimension, extent along the
// contiguous index and base address a multiple of 4 floats -- checked by the launchers); the scalar
// variant (one predicated 4-byte load per element) remains for the 10- / 24-wide heads.
template <int MODE, int BN, bool VEC>
__device__ __forceinline__ void bwd_gemm_body(const BwdGemmK& p, const int bx, const int by, const int bz, const int gz,
                                              const DetAcc& det) {      // det: deterministic accumulation of the atomic stores, or all null
  constexpr int NT = BN / 16;
  constexpr int AE = 64 * BG_RK / 256;      // A elements per thread and step (8)
  constexpr int BE = BN * BG_RK / 256;      // B elements per thread and step (8 or 4)
  constexpr int LDA_D = BG_RK + 1;          // DATA:   As[i][r]
  constexpr int LDA_W = 64 + 16;            // WEIGHT: As[r][i]
  constexpr int LDB = BN + 16;
  __shared__ __align__(16) float As[(64 * LDA_D > BG_RK * LDA_W) ? 64 * LDA_D : BG_RK * LDA_W];
  __shared__ __align__(16) float Bs[BG_RK * LDB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i0 = by * 64, j0 = bx * BN;
  const int rbeg = bz * p.rchunk, rend = min(p.R, rbeg + p.rchunk);
  f32x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  float csum = 0.f;
  const bool do_colsum = MODE == BWD_WEIGHT && p.colsum != nullptr && bx == 0;
  float ra[AE], rb[BE];

  auto fetch = [&](int r0) {
    if constexpr (VEC) {
      // A: 4 consecutive elements along the contiguous index (DATA: r, WEIGHT: i)
#pragma unroll
      for (int e = 0; e < AE / 4; ++e) {
        const int idx = tid + 256 * e;
        int i, r;
        if (MODE == BWD_DATA) { r = (idx & (BG_RK / 4 - 1)) * 4; i = idx / (BG_RK / 4); }
        else { i = (idx & 15) * 4; r = idx >> 4; }
        const int gi = i0 + i, gr = r0 + r;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (gi < p.I && gr < rend) {            // extents are multiples of 4: the four are in or out together
          const size_t off = MODE == BWD_DATA ? (size_t)gi * p.ldA + gr : (size_t)gr * p.ldA + gi;
          v = ld4(p.A + off);
          if (p.relu != nullptr) {
            const float4 m = ld4(p.relu + off);
            if (m.x <= 0.f) v.x = 0.f;
            if (m.y <= 0.f) v.y = 0.f;
            if (m.z <= 0.f) v.z = 0.f;
            if (m.w <= 0.f) v.w = 0.f;
          }
          if (p.gate != nullptr) {
            if (MODE == BWD_DATA) { if (p.gate[gi] <= 0) v = make_float4(0.f, 0.f, 0.f, 0.f); }
            else if (p.gate[gr] <= 0) v = make_float4(0.f, 0.f, 0.f, 0.f);
          }
        }
        ra[4 * e] = v.x; ra[4 * e + 1] = v.y; ra[4 * e + 2] = v.z; ra[4 * e + 3] = v.w;
      }
#pragma unroll
      for (int e = 0; e < BE / 4; ++e) {
        const int idx = tid + 256 * e;
        const int j = (idx % (BN / 4)) * 4, r = idx / (BN / 4);
        const int gj = j0 + j, gr = r0 + r;
        const float4 v = (gj < p.J && gr < rend) ? ld4(p.Bm + (size_t)gr * p.ldB + gj) : make_float4(0.f, 0.f, 0.f, 0.f);
        rb[4 * e] = v.x; rb[4 * e + 1] = v.y; rb[4 * e + 2] = v.z; rb[4 * e + 3] = v.w;
      }
    } else {
#pragma unroll
      for (int e = 0; e < AE; ++e) {
        const int idx = tid + 256 * e;
        int i, r;
        if (MODE == BWD_DATA) { r = idx & (BG_RK - 1); i = idx / BG_RK; }
        else { i = idx & 63; r = idx >> 6; }
        ra[e] = bg_load_a<MODE>(p, i0 + i, r0 + r, rend);
      }
#pragma unroll
      for (int e = 0; e < BE; ++e) {
        const int idx = tid + 256 * e;
        const int j = idx % BN, r = idx / BN;
        const int gj = j0 + j, gr = r0 + r;
        rb[e] = (gj < p.J && gr < rend) ? p.Bm[(size_t)gr * p.ldB + gj] : 0.f;
      }
    }
  };
  auto stage = [&]() {
    if constexpr (VEC) {
#pragma unroll
      for (int e = 0; e < AE / 4; ++e) {
        const int idx = tid + 256 * e;
        if (MODE == BWD_DATA) {
          float* d = &As[(idx / (BG_RK / 4)) * LDA_D + (idx & (BG_RK / 4 - 1)) * 4];     // row stride 33: scalar stores
          d[0] = ra[4 * e]; d[1] = ra[4 * e + 1]; d[2] = ra[4 * e + 2]; d[3] = ra[4 * e + 3];
        } else {
          *reinterpret_cast<float4*>(&As[(idx >> 4) * LDA_W + (idx & 15) * 4]) =
              make_float4(ra[4 * e], ra[4 * e + 1], ra[4 * e + 2], ra[4 * e + 3]);
        }
      }
#pragma unroll
      for (int e = 0; e < BE / 4; ++e) {
        const int idx = tid + 256 * e;
        *reinterpret_cast<float4*>(&Bs[(idx / (BN / 4)) * LDB + (idx % (BN / 4)) * 4]) =
            make_float4(rb[4 * e], rb[4 * e + 1], rb[4 * e + 2], rb[4 * e + 3]);
      }
    } else {
#pragma unroll
      for (int e = 0; e < AE; ++e) {
        const int idx = tid + 256 * e;
        if (MODE == BWD_DATA) As[(idx / BG_RK) * LDA_D + (idx & (BG_RK - 1))] = ra[e];
        else As[(idx >> 6) * LDA_W + (idx & 63)] = ra[e];
      }
#pragma unroll
      for (int e = 0; e < BE; ++e) {
        const int idx = tid + 256 * e;
        Bs[(idx / BN) * LDB + idx % BN] = rb[e];
      }
    }
  };

  fetch(rbeg);
  for (int r0 = rbeg; r0 < rend; r0 += BG_RK) {
    stage();
    __syncthreads();
    if (r0 + BG_RK < rend) fetch(r0 + BG_RK);
    if (do_colsum && tid < 64) {
#pragma unroll
      for (int r = 0; r < BG_RK; ++r) csum += As[r * LDA_W + tid];
    }
#pragma unroll
    for (int kk = 0; kk < BG_RK / 4; ++kk) {
      const int k = 4 * kk + (lane >> 4);
      const int ai = 16 * wave + (lane & 15);
      const float a = MODE == BWD_DATA ? As[ai * LDA_D + k] : As[k * LDA_W + ai];
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = MFMA4(a, Bs[k * LDB + 16 * t + (lane & 15)], acc[t]);
    }
    __syncthreads();
  }
  const bool atomic = MODE == BWD_WEIGHT || gz > 1;
  long long* const sC = atomic ? det_shadow_of(det, p.C) : nullptr;      // (C lies inside one range or outside both)
  if (sC != nullptr) {           // deterministic mode (wave-uniform): integer atomics on the shadow of C
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int col = j0 + 16 * t + (lane & 15);
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int row = i0 + 16 * wave + 4 * (lane >> 4) + reg;
        if (row < p.I && col < p.J) {
          float v = acc[t][reg] * p.alpha;
          if (p.cmask != nullptr && p.cmask[(size_t)row * p.ldC + col] <= 0.f) v = 0.f;
          acc_add_at(sC + ((size_t)row * p.ldC + col), p.C + (size_t)row * p.ldC + col, v);
        }
      }
    }
  } else {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int col = j0 + 16 * t + (lane & 15);
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int row = i0 + 16 * wave + 4 * (lane >> 4) + reg;
        if (row < p.I && col < p.J) {
          float v = acc[t][reg] * p.alpha;
          float* c = p.C + (size_t)row * p.ldC + col;
          if (p.cmask != nullptr && p.cmask[(size_t)row * p.ldC + col] <= 0.f) v = 0.f;
          if (atomic) unsafeAtomicAdd(c, v);
          else if (p.accumulate) *c += v;
          else *c = v;
        }
      }
    }
  }
  if (do_colsum && tid < 64 && i0 + tid < p.I) acc_add_at(det_shadow_of(det, p.colsum + i0 + tid), p.colsum + i0 + tid, csum);
}

template <int MODE, int BN, bool VEC>
__global__ __launch_bounds__(256) void bwd_gemm_kernel(BwdGemmK p, DetAcc det) {
  bwd_gemm_body<MODE, BN, VEC>(p, blockIdx.x, blockIdx.y, blockIdx.z, gridDim.z, det);
}

// Every weight gradient of an iteration in ONE launch (two: the 16-byte-load variant and the scalar one for the
// 10-wide heads): dW_i += dY_i^T X_i, db_i += colsum dY_i.  The items travel in the kernel-argument segment, a
// block finds its item from the block offsets.  (Round 2: one launch per weight, 37 per iteration, ~10 us each
// for a 900 x 256 x 256 product.)
constexpr int WGROUP_MAX = 48;
struct WGroupItem { BwdGemmK p; int first_block, gx, gy, gz; };
struct WGroupK { WGroupItem it[WGROUP_MAX]; int n; DetAcc det; };
template <bool VEC>
__global__ __launch_bounds__(256) void bwd_weight_group_kernel(WGroupK g) {
  int i = 0;
#pragma unroll 1
  for (int j = 1; j < g.n; ++j)
    if ((int)blockIdx.x >= g.it[j].first_block) i = j;
  const WGroupItem& it = g.it[i];
  int b = (int)blockIdx.x - it.first_block;
  const int bx = b % it.gx; b /= it.gx;
  const int by = b % it.gy;
  const int bz = b / it.gy;
  bwd_gemm_body<BWD_WEIGHT, 64, VEC>(it.p, bx, by, bz, it.gz, g.det);
}

static bool bg_vec_ok(const BwdGemmK& p, int contiguous_a_extent) {
  auto al = [](const void* q) { return (reinterpret_cast<size_t>(q) & 15) == 0; };
  return (p.ldA & 3) == 0 && (p.ldB & 3) == 0 && (p.J & 3) == 0 && (contiguous_a_extent & 3) == 0 &&
         al(p.A) && al(p.Bm) && (p.relu == nullptr || al(p.relu));
}

int launch_linear_bwd_data(const float* dy, const float* relu_out, const int* row_gate,
                           const float* w, const float* in_relu_mask, float* dx, int M, int K,
                           int N, float alpha, int accumulate, hipStream_t s) {
  TC_REQUIRE(M > 0 && K > 0 && N > 0, "linear_bwd_data: M=%d K=%d N=%d", M, K, N);
  BwdGemmK p;
  const DetAcc det = current_det();
  p.A = dy; p.relu = relu_out; p.gate = row_gate; p.Bm = w; p.cmask = in_relu_mask; p.C = dx;
  p.colsum = nullptr; p.ldA = N; p.ldB = K; p.ldC = K; p.I = M; p.J = K; p.R = N;
  p.rchunk = ((N + BG_RK - 1) / BG_RK) * BG_RK; p.accumulate = accumulate; p.alpha = alpha;
  const int mt = (M + 63) / 64;
  const bool vec = bg_vec_ok(p, N);         // A = dY[m][n]: contiguous along the reduction index n
  const bool wide = mt * ((K + 63) / 64) >= 200;          // enough 64-wide tiles to fill the chip
  // A few dozen workgroups that each walk a long reduction (the token side of the fused backward: 256 rows, dK|dV ->
  // dmem over n = 512: 32 workgroups x 16 k-steps = 14 us of latency): when the result is ADDED to dx anyway, split
  // the reduction over gz workgroups that add their parts with float atomics (round 4: 3 x 14 -> 3 x 6 us)
  int gz = 1;
  // (deterministic mode: no split -- a single writer per element adds in place)
  if (accumulate && !wide && mt * ((K + 31) / 32) <= 64 && N >= 256 && det.shadow[0] == nullptr && det.shadow[1] == nullptr) {
    gz = N >= 512 ? 4 : 2;
    p.rchunk = (((N + gz - 1) / gz + BG_RK - 1) / BG_RK) * BG_RK;
    gz = (N + p.rchunk - 1) / p.rchunk;
  }
  const dim3 grid(wide ? (K + 63) / 64 : (K + 31) / 32, mt, gz);
  if (wide && vec) hipLaunchKernelGGL((bwd_gemm_kernel<BWD_DATA, 64, true>), grid, dim3(256), 0, s, p, det);
  else if (wide) hipLaunchKernelGGL((bwd_gemm_kernel<BWD_DATA, 64, false>), grid, dim3(256), 0, s, p, det);
  else if (vec) hipLaunchKernelGGL((bwd_gemm_kernel<BWD_DATA, 32, true>), grid, dim3(256), 0, s, p, det);
  else hipLaunchKernelGGL((bwd_gemm_kernel<BWD_DATA, 32, false>), grid, dim3(256), 0, s, p, det);
  return check_launch("linear_bwd_data");
}

int launch_linear_bwd_weight(const float* x, const float* dy, const float* relu_out,
                             const int* row_gate, float* dw, float* db, int M, int K, int N,
                             float alpha, hipStream_t s) {
  TC_REQUIRE(M > 0 && K > 0 && N > 0, "linear_bwd_weight: M=%d K=%d N=%d", M, K, N);
  BwdGemmK p;
  const DetAcc det = current_det();
  p.A = dy; p.relu = relu_out; p.gate = row_gate; p.Bm = x; p.cmask = nullptr; p.C = dw;
  p.colsum = db; p.ldA = N; p.ldB = K; p.ldC = K; p.I = N; p.J = K; p.R = M;
  p.rchunk = 64; p.accumulate = 1; p.alpha = alpha;
  TC_REQUIRE(dw != nullptr, "linear_bwd_weight: dw is NULL");
  const dim3 grid((K + 63) / 64, (N + 63) / 64, (M + p.rchunk - 1) / p.rchunk);
  if (bg_vec_ok(p, N))                      // A = dY[m][n]: contiguous along the output row index n
    hipLaunchKernelGGL((bwd_gemm_kernel<BWD_WEIGHT, 64, true>), grid, dim3(256), 0, s, p, det);
  else
    hipLaunchKernelGGL((bwd_gemm_kernel<BWD_WEIGHT, 64, false>), grid, dim3(256), 0, s, p, det);
  return check_launch("linear_bwd_weight");
}

int launch_linear_bwd_weight_group(const WeightJob* jobs, int n, hipStream_t s) {
  TC_REQUIRE(n >= 1 && n <= WGROUP_MAX, "linear_bwd_weight_group: %d items (1..%d)", n, WGROUP_MAX);
  WGroupK g[2];                      // [1]: 16-byte operand loads, [0]: scalar
  int blocks[2] = {0, 0};
  g[0].n = g[1].n = 0;
  g[0].det = g[1].det = current_det();
  for (int i = 0; i < n; ++i) {
    const WeightJob& j = jobs[i];
    TC_REQUIRE(j.M > 0 && j.K > 0 && j.N > 0 && j.dw != nullptr && j.x != nullptr && j.dy != nullptr,
               "linear_bwd_weight_group: bad item %d", i);
    BwdGemmK p;
    p.A = j.dy; p.relu = j.relu; p.gate = nullptr; p.Bm = j.x; p.cmask = nullptr; p.C = j.dw;
    p.colsum = j.db; p.ldA = j.N; p.ldB = j.ldx > 0 ? j.ldx : j.K; p.ldC = j.K; p.I = j.N; p.J = j.K; p.R = j.M;
#ifndef TC_WG_RCHUNK
#define TC_WG_RCHUNK 256     // rows per workgroup: 128 -> 256 halved the float atomics into dW (0.845 -> 0.809 ms per iteration; 512: the same)
#endif
    p.rchunk = TC_WG_RCHUNK; p.accumulate = 1; p.alpha = 1.0f;
    const int v = bg_vec_ok(p, j.N) ? 1 : 0;
    WGroupItem& it = g[v].it[g[v].n++];
    it.p = p; it.gx = (j.K + 63) / 64; it.gy = (j.N + 63) / 64; it.gz = (j.M + p.rchunk - 1) / p.rchunk;
    it.first_block = blocks[v];
    blocks[v] += it.gx * it.gy * it.gz;
  }
  if (g[1].n > 0) hipLaunchKernelGGL((bwd_weight_group_kernel<true>), dim3(blocks[1]), dim3(256), 0, s, g[1]);
  if (g[0].n > 0) hipLaunchKernelGGL((bwd_weight_group_kernel<false>), dim3(blocks[0]), dim3(256), 0, s, g[0]);
  return check_launch("linear_bwd_weight_group");
}

// ---- deterministic accumulation: the calling thread's scope and the flush ---------------------------------------
DetAcc& current_det() {
  static thread_local DetAcc d = {{nullptr, nullptr}, {nullptr, nullptr}, {nullptr, nullptr}};
  return d;
}
DetAcc*& current_det_device() {
  static thread_local DetAcc* p = nullptr;
  return p;
}
__global__ __launch_bounds__(256) void det_flush_kernel(float* dst, long long* shadow, size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const long long v = shadow[i];
    if (v != 0) {
      dst[i] += (float)((double)v * (1.0 / (double)DET_SCALE));
      shadow[i] = 0;
    }
  }
}
__global__ void det_store_kernel(DetAcc d, DetAcc* dst) { *dst = d; }
int launch_det_store(const DetAcc& d, DetAcc* dst, hipStream_t s) {
  hipLaunchKernelGGL(det_store_kernel, dim3(1), dim3(1), 0, s, d, dst);
  return check_launch("det_store");
}
int launch_det_flush(const DetAcc& d, int range, hipStream_t s) {
  TC_REQUIRE(range >= 0 && range < 2, "det_flush: range %d", range);
  if (d.shadow[range] == nullptr) return 0;
  const size_t n = (size_t)(d.hi[range] - d.lo[range]);
  if (n == 0) return 0;
  const int grid = (int)std::min<size_t>((n + 255) / 256, 2048);
  hipLaunchKernelGGL(det_flush_kernel, dim3(grid), dim3(256), 0, s, const_cast<float*>(d.lo[range]), d.shadow[range], n);
  return check_launch("det_flush");
}

// ---- LayerNorm(a (+b)) (+ReLU) backward, C = 256 ---------------------------
struct LnBwdK {
  const float* a; const float* b; const float* gamma; const float* dy; const float* relu_out;
  float* dz; float* dgamma; float* dbeta; int M;
  DetAcc det;
};

__global__ __launch_bounds__(256) void ln_bwd_kernel(LnBwdK p) {
  __shared__ float4 sg[4][64];
  __shared__ float4 sb[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float4 g = ld4(p.gamma + 4 * lane);
  float4 ag = make_float4(0.f, 0.f, 0.f, 0.f), ab = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int row = blockIdx.x * 4 + wave; row < p.M; row += gridDim.x * 4) {
    const size_t o = (size_t)row * 256 + 4 * lane;
    float4 z = ld4(p.a + o);
    if (p.b != nullptr) { const float4 t = ld4(p.b + o); z.x += t.x; z.y += t.y; z.z += t.z; z.w += t.w; }
    // same statistics as the forward (rowdev.hpp ln_row)
    const float mean = wave_sum(z.x + z.y + z.z + z.w) * (1.0f / 256.0f);
    const float4 d = make_float4(z.x - mean, z.y - mean, z.z - mean, z.w - mean);
    const float q = wave_sum(d.x * d.x + d.y * d.y + d.z * d.z + d.w * d.w);
    const float rstd = 1.0f / sqrtf(q * (1.0f / 256.0f) + 1e-5f);
    const float4 xh = make_float4(d.x * rstd, d.y * rstd, d.z * rstd, d.w * rstd);
    float4 dy = ld4(p.dy + o);
    if (p.relu_out != nullptr) {
      const float4 y = ld4(p.relu_out + o);
      if (y.x <= 0.f) dy.x = 0.f;
      if (y.y <= 0.f) dy.y = 0.f;
      if (y.z <= 0.f) dy.z = 0.f;
      if (y.w <= 0.f) dy.w = 0.f;
    }
    ag.x += dy.x * xh.x; ag.y += dy.y * xh.y; ag.z += dy.z * xh.z; ag.w += dy.w * xh.w;
    ab.x += dy.x; ab.y += dy.y; ab.z += dy.z; ab.w += dy.w;
    const float4 dx = make_float4(dy.x * g.x, dy.y * g.y, dy.z * g.z, dy.w * g.w);
    const float s1 = wave_sum(dx.x + dx.y + dx.z + dx.w) * (1.0f / 256.0f);
    const float s2 = wave_sum(dx.x * xh.x + dx.y * xh.y + dx.z * xh.z + dx.w * xh.w) * (1.0f / 256.0f);
    st4(p.dz + o, make_float4(rstd * (dx.x - s1 - xh.x * s2), rstd * (dx.y - s1 - xh.y * s2),
                              rstd * (dx.z - s1 - xh.z * s2), rstd * (dx.w - s1 - xh.w * s2)));
  }
  sg[wave][lane] = ag; sb[wave][lane] = ab;
  __syncthreads();
  if (wave == 0) {
    float4 tg = sg[0][lane], tb = sb[0][lane];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      tg.x += sg[w][lane].x; tg.y += sg[w][lane].y; tg.z += sg[w][lane].z; tg.w += sg[w][lane].w;
      tb.x += sb[w][lane].x; tb.y += sb[w][lane].y; tb.z += sb[w][lane].z; tb.w += sb[w][lane].w;
    }
    if (p.dgamma != nullptr) {
      float* dg = p.dgamma + 4 * lane;
      long long* sp = det_shadow_of(p.det, dg);
      acc_add_at(sp, dg, tg.x); acc_add_at(sp ? sp + 1 : sp, dg + 1, tg.y);
      acc_add_at(sp ? sp + 2 : sp, dg + 2, tg.z); acc_add_at(sp ? sp + 3 : sp, dg + 3, tg.w);
    }
    if (p.dbeta != nullptr) {
      float* dbp = p.dbeta + 4 * lane;
      long long* sp = det_shadow_of(p.det, dbp);
      acc_add_at(sp, dbp, tb.x); acc_add_at(sp ? sp + 1 : sp, dbp + 1, tb.y);
      acc_add_at(sp ? sp + 2 : sp, dbp + 2, tb.z); acc_add_at(sp ? sp + 3 : sp, dbp + 3, tb.w);
    }
  }
}

int launch_ln256_bwd(const float* a, const float* b, const float* gamma, const float* dy,
                     const float* relu_out, float* dz, float* dgamma, float* dbeta, int M,
                     hipStream_t s) {
  TC_REQUIRE(M > 0, "layernorm_bwd: M=%d", M);
  LnBwdK p;
  p.det = current_det();
  p.a = a; p.b = b; p.gamma = gamma; p.dy = dy; p.relu_out = relu_out; p.dz = dz;
  p.dgamma = dgamma; p.dbeta = dbeta; p.M = M;
  const int grid = min((M + 3) / 4, 64);   // few workgroups: dgamma/dbeta meet in 512 atomics each
  hipLaunchKernelGGL(ln_bwd_kernel, dim3(grid), dim3(256), 0, s, p);
  return check_launch("layernorm_bwd");
}

// ---- gated radar attention core, backward ----------------------------------
struct RadBwdK {
  const float* qproj; const float* kv; const float* cxy; const float* box; const float* rxy;
  const float* attn_out; const float* d_attn;
  int ldq, ldkv, code, ld_xy, ld_c, B, Q, T, pad_mult;
  int lph;                     // lanes per head: 64 / heads
  float rmin, rmax, qscale;
  float* dq; float* dkv;
  DropK drop;                  // dropout on the attention probabilities (thr 0 = off)
  DetAcc det;
};

__global__ __launch_bounds__(256) void radar_attn_bwd_kernel(RadBwdK p) {
  const int lane = threadIdx.x & 63;
  const int row = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
  if (row >= p.B * p.Q) return;
  const int b = row / p.Q;
  const float cx = p.cxy[(size_t)row * p.ld_c + 0], cy = p.cxy[(size_t)row * p.ld_c + 1];
  const float* bx = p.box + (size_t)row * p.code;
  float4 q4 = ld4(p.qproj + (size_t)row * p.ldq + 4 * lane);
  q4.x *= p.qscale; q4.y *= p.qscale; q4.z *= p.qscale; q4.w *= p.qscale;
  const float4 dO = ld4(p.d_attn + (size_t)row * 256 + 4 * lane);
  const float4 o4 = ld4(p.attn_out + (size_t)row * 256 + 4 * lane);
  const float4 dq = radar_attn_bwd_row(cx, cy, bx[3], bx[6], bx[7], p.rmin, p.rmax, q4,
                                       p.rxy + (size_t)b * p.T * p.ld_xy, p.ld_xy, p.kv + (size_t)b * p.T * p.ldkv,
                                       p.dkv + (size_t)b * p.T * p.ldkv, p.ldkv, p.T, p.pad_mult, dO, o4, p.drop, row, lane,
                                       p.lph, det_shadow_of(p.det, p.dkv + (size_t)b * p.T * p.ldkv));
  st4(p.dq + (size_t)row * 256 + 4 * lane,
      make_float4(dq.x * p.qscale, dq.y * p.qscale, dq.z * p.qscale, dq.w * p.qscale));
}

int launch_radar_attn_bwd(const RadarAttnArgs& a, float qscale, const float* d_attn, float* dq,
                          float* dkv, hipStream_t s) {
  TC_REQUIRE(a.C == 256 && heads_ok(a.H), "radar_attn_bwd: C=%d num_heads=%d (256 with 4, 8 or 16 heads supported)", a.C, a.H);
  TC_REQUIRE(a.T > 0 && a.pad_mult >= 1, "radar_attn_bwd: T=%d pad_mult=%d", a.T, a.pad_mult);
  RadBwdK p;
  p.qproj = a.qproj; p.kv = a.kv; p.cxy = a.centre_xy; p.box = a.box; p.rxy = a.radar_xy;
  p.attn_out = a.attn_out; p.d_attn = d_attn;
  p.ldq = a.ldq; p.ldkv = a.ldkv; p.code = a.code; p.ld_xy = a.ld_xy; p.ld_c = a.ld_c;
  p.B = a.B; p.Q = a.Q; p.T = a.T; p.pad_mult = a.pad_mult; p.rmin = a.rmin; p.rmax = a.rmax;
  p.lph = 64 / a.H;
  p.qscale = qscale; p.dq = dq; p.dkv = dkv; p.drop = a.drop; p.det = current_det();
  const int rows = a.B * a.Q;
  hipLaunchKernelGGL(radar_attn_bwd_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, p);
  return check_launch("radar_attn_bwd");
}

// ---- elementwise dropout: out = (res) + [gate] * keep * x / (1 - p) -----------
// forward of rf_dropout / rf_dropout2 / rf_dropout3 (HEAD:581-585) and, applied to the
// gradient with the same (seed, site), their backward.  Element index row * cols + col.
__global__ void dropout_kernel(const float* x, const float* res, const int* gate, int rows, int cols,
                               DropK d, float* out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)rows * cols) return;
  float v = drop_keep(d.seed, d.site, (unsigned)i, d.thr) ? x[i] * d.scale : 0.0f;
  if (gate != nullptr && gate[i / cols] <= 0) v = 0.0f;
  out[i] = res != nullptr ? res[i] + v : v;
}
int launch_dropout(const float* x, const float* res, const int* gate, int rows, int cols, const DropK& d,
                   float* out, hipStream_t s) {
  const size_t n = (size_t)rows * cols;
  TC_REQUIRE(n > 0 && n < (1ull << 32), "dropout: %d x %d elements", rows, cols);
  hipLaunchKernelGGL(dropout_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, res, gate, rows,
                     cols, d, out);
  return check_launch("dropout");
}

// ---- box = reg_out (+ reference): backward into the previous layer's box ----
// HEAD:661-665: tmp2[0:2] += new_reference_3d[0:2] (= tmp[0:2]), tmp2[4] += tmp[4]
__global__ void box_ref_bwd_kernel(const float* d_box, int code, float* d_prev, int M) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M) return;
  const float* d = d_box + (size_t)i * code;
  float* o = d_prev + (size_t)i * code;
  o[0] += d[0]; o[1] += d[1]; o[4] += d[4];
}

int launch_box_ref_bwd(const float* d_box, int code, float* d_prev, int M, hipStream_t s) {
  TC_REQUIRE(M > 0 && code >= 5, "box_ref_bwd: M=%d code=%d", M, code);
  hipLaunchKernelGGL(box_ref_bwd_kernel, dim3((M + 255) / 256), dim3(256), 0, s, d_box, code, d_prev, M);
  return check_launch("box_ref_bwd");
}

// ---- optimizer on the flat gradient bucket ----------------------------------
// sum of squares; the clip coefficient stays on the device.
// DETERMINISTIC (round 3): the ranks of a data-parallel job evaluate this on the SAME all-reduced bucket and must get
// the same clip coefficient bit for bit, or the replicas drift apart (a two-rank test found 1.7e-10 relative after
// three steps with the block sums meeting in float atomics).  out[] is TC_SQ_NORM_PARTIALS slots: workgroup b adds
// the sum over the elements it owns to out[b] (its own slot: no atomics, a fixed order inside the workgroup);
// adamw_kernel adds the slots up in index order -- the launch boundary is the hand-off, no fence, no ticket.
constexpr int SQ_NT = 1024;
static_assert(TC_SQ_NORM_PARTIALS == 256, "adamw_kernel reads one slot per thread");
__global__ __launch_bounds__(SQ_NT) void sqnorm_kernel(const float* g, size_t n, float* out) {
  __shared__ float red[SQ_NT / 64];
  float acc = 0.f;
  const size_t n4 = (reinterpret_cast<uintptr_t>(g) & 15) == 0 ? n / 4 : 0;
  const float4* g4 = reinterpret_cast<const float4*>(g);
  for (size_t i = (size_t)blockIdx.x * SQ_NT + threadIdx.x; i < n4; i += (size_t)gridDim.x * SQ_NT) {
    const float4 v = g4[i];
    acc += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
  }
  for (size_t i = 4 * n4 + (size_t)blockIdx.x * SQ_NT + threadIdx.x; i < n; i += (size_t)gridDim.x * SQ_NT) {
    const float v = g[i];
    acc += v * v;
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < SQ_NT / 64; ++i) t += red[i];
    out[blockIdx.x] += t;
  }
}

int launch_sqnorm(const float* g, size_t n, float* out, hipStream_t s) {
  TC_REQUIRE(n > 0, "sqnorm: n=0");
  hipLaunchKernelGGL(sqnorm_kernel, dim3(TC_SQ_NORM_PARTIALS), dim3(SQ_NT), 0, s, g, n, out);
  return check_launch("sqnorm");
}

// torch.optim.AdamW step (decoupled weight decay) with mmcv's grad clip
// (clip_grad_norm_: coef = max_norm / (norm + 1e-6), applied when < 1) and the
// 1/world_size of the gradient all-reduce folded in.  sum(sqnorm[0 .. TC_SQ_NORM_PARTIALS)) = sum g^2 of
// the already averaged gradient when grad_scale == 1, else of the raw sum.
struct AdamK {
  float* p; const float* g; float* m; float* v; size_t n;
  float lr, b1, b2, eps, wd, bc1, bc2, grad_scale, max_norm;
  const float* sqnorm;
};

__global__ __launch_bounds__(256) void adamw_kernel(AdamK a) {
  float coef = a.grad_scale;
  if (a.sqnorm != nullptr && a.max_norm > 0.f) {
    // every workgroup adds the slots up itself, in the same order (TC_SQ_NORM_PARTIALS == its 256 threads)
    __shared__ float red[4];
    const float part = wave_sum(a.sqnorm[threadIdx.x]);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = part;
    __syncthreads();
    const float norm = sqrtf((red[0] + red[1]) + (red[2] + red[3])) * a.grad_scale;
    const float c = a.max_norm / (norm + 1e-6f);
    if (c < 1.0f) coef *= c;
  }
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (size_t)gridDim.x * 256) {
    const float g = a.g[i] * coef;
    float pv = a.p[i];
    pv *= 1.0f - a.lr * a.wd;
    const float m = a.b1 * a.m[i] + (1.0f - a.b1) * g;
    const float v = a.b2 * a.v[i] + (1.0f - a.b2) * g * g;
    a.m[i] = m; a.v[i] = v;
    const float denom = sqrtf(v) / sqrtf(a.bc2) + a.eps;
    a.p[i] = pv - (a.lr / a.bc1) * (m / denom);
  }
}

int launch_adamw(float* p, const float* g, float* m, float* v, size_t n, float lr, float b1,
                 float b2, float eps, float wd, int step, float grad_scale, float max_norm,
                 const float* sqnorm, hipStream_t s) {
  TC_REQUIRE(n > 0 && step >= 1, "adamw: n=%zu step=%d", n, step);
  AdamK a;
  a.p = p; a.g = g; a.m = m; a.v = v; a.n = n; a.lr = lr; a.b1 = b1; a.b2 = b2; a.eps = eps;
  // the bias corrections in double, as torch forms them from Python floats: in float, b2^step rounds at 6e-8 and
  // 1 - b2^step is ~1e-3 x step in the first steps, so bc2 was off by up to 1.5e-5 of itself there (2.5e-6 of the
  // update at step 2, measured against fp64 on a single parameter: tests/test_gpu_loss_kernels.py)
  a.wd = wd;
  a.bc1 = (float)(1.0 - std::pow((double)b1, (double)step));
  a.bc2 = (float)(1.0 - std::pow((double)b2, (double)step));
  a.grad_scale = grad_scale; a.max_norm = max_norm; a.sqnorm = sqnorm;
  const int grid = (int)min((n + 255) / 256, (size_t)2048);
  hipLaunchKernelGGL(adamw_kernel, dim3(grid), dim3(256), 0, s, a);
  return check_launch("adamw");
}

}  // namespace tc
