// NMS-free box decoding (CODER:39-90, UTIL:26-52, HEAD:1018): sigmoid, top-300
// of the 9000 (query, class) scores, gather + denormalise, centre-range mask,
// z -= h/2.  One workgroup per sample; a key is 64 bits (score bits << 32 | ~index), so keys are
// unique and an 8-bit radix SELECT finds the max_num-th largest exactly.  Ties resolve to the lower
// flat index (torch.topk leaves tie order unspecified).  <1 % of the frame, but 4 % of the one-frame
// latency path when it took 20 us (round 2: four barriers and a one-wave scan per pass, 300 atomics on
// one LDS word, a 45-stage bitonic sort of 512 keys behind 16 waves' barriers).  Round 3:
//   * a thread's <= 12 keys stay in registers; the eight passes' histograms are separate (zeroed once):
//     ONE barrier per pass, every wave does the 256-bin scan itself (no broadcast through LDS);
//   * the survivors are compacted with one atomic per wave-instruction and ordered by RANK
//     (rank = the number of larger survivors: two threads per survivor, 16-byte LDS reads) -- one barrier.
// Beyond 12 288 scores or max_num 512 (a 26-class head, 1 300 queries, max_num = 1000): box_decode_stream_kernel below,
// the same key and select without the registers; launch_box_decode picks by shape.
#include "kernels.hpp"

namespace tc {

constexpr int DEC_THREADS = 1024;
constexpr int DEC_MAXN = 12288;   // Q * num_classes upper bound
constexpr int DEC_NK = DEC_MAXN / DEC_THREADS;
constexpr int DEC_MAXK = 512;
constexpr int DEC_PASSES = 9;     // the bucket pass + up to eight byte passes (bit 63 = the score's sign = 0)

struct DecK {
  const float* cls; const float* box; int Q, ncls, code, K;
  float pcr[6];
  float* boxes; float* scores; int* labels; unsigned char* valid;      // fixed-size rows + mask (may be null)
  // round 4: the rows NMSFreeCoder keeps (inside post_center_range, above the score threshold), compacted in score
  // order, and their number -- what decode_single returns (CODER:66-84) without a mask select on the host side
  float* kboxes; float* kscores; long long* klabels; int* kcount;      // (may be null)
  float thr; int use_thr; int z_shift;
};

#ifdef TC_CHAIN_STAMPS
__device__ long long g_dec_stamps[16];
#define DEC_STAMP(i) do { if (blockIdx.x == 0 && threadIdx.x == 0) g_dec_stamps[i] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define DEC_STAMP(i) do {} while (0)
#endif

struct DecLds {
  alignas(16) unsigned int hist[DEC_PASSES][256];
  alignas(16) unsigned long long sel[DEC_MAXK];      // survivors, any order; zero behind them
  unsigned int rank[DEC_MAXK];                       // survivor -> its place in descending order
  unsigned long long keep[DEC_MAXK / 64];            // bit i: output row i is kept
  unsigned int count, ccount;
};

__device__ __forceinline__ unsigned bucket(unsigned long long k) { return (unsigned)min(max((int)(k >> 51) - 1776, 0), 255); }

// inclusive prefix sum over the 64 lanes (row_shr 1, 2, 4, 8; row_bcast 15 / 31), integers
template <int CTRL, int ROWS>
__device__ __forceinline__ int dpp_iadd(int v) { return v + __builtin_amdgcn_update_dpp(0, v, CTRL, ROWS, 0xF, false); }
__device__ __forceinline__ int wave_scan_incl(int v) {
  v = dpp_iadd<0x111, 0xF>(v); v = dpp_iadd<0x112, 0xF>(v); v = dpp_iadd<0x114, 0xF>(v); v = dpp_iadd<0x118, 0xF>(v);
  v = dpp_iadd<0x142, 0xA>(v); v = dpp_iadd<0x143, 0xC>(v);
  return v;
}

__global__ __launch_bounds__(DEC_THREADS) void box_decode_kernel(DecK p) {
  __shared__ DecLds S;
  extern __shared__ __align__(16) unsigned long long cand[];     // [Q * num_classes] the K-th key's bucket
  DEC_STAMP(0);
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int n = p.Q * p.ncls;
  const float* cls = p.cls + (size_t)b * n;
  float logit[DEC_NK];
#pragma unroll
  for (int j = 0; j < DEC_NK; ++j) {
    const int i = tid + j * DEC_THREADS;
    logit[j] = i < n ? cls[i] : 0.0f;
  }
  // (under the loads)
  for (int i = tid; i < DEC_PASSES * 256; i += DEC_THREADS) (&S.hist[0][0])[i] = 0u;
  for (int i = tid; i < DEC_MAXK; i += DEC_THREADS) { S.sel[i] = 0ull; S.rank[i] = 0u; }
  if (tid == 0) { S.count = 0u; S.ccount = 0u; }
  if (tid < DEC_MAXK / 64) S.keep[tid] = 0ull;
  unsigned long long key[DEC_NK];
#pragma unroll
  for (int j = 0; j < DEC_NK; ++j) {
    const int i = tid + j * DEC_THREADS;
    // sigmoid in [0, 1]: the bit pattern is order preserving.  0 marks "no key" (a real key's low word is ~i != 0)
    key[j] = i < n ? ((unsigned long long)__float_as_uint(sigmoidf_(logit[j])) << 32) | (unsigned int)(0xFFFFFFFFu - (unsigned)i)
                   : 0ull;
  }
  __syncthreads();                                    // histograms zeroed
  DEC_STAMP(1);
#pragma unroll
  for (int j = 0; j < DEC_NK; ++j)
    if (key[j] != 0ull) atomicAdd(&S.hist[0][bucket(key[j])], 1u);
  __syncthreads();
  DEC_STAMP(2);
  const int K = min(p.K, n);
  // radix select: the K-th largest key.
  // Pass 0 does NOT look at a bit field: the exponent byte of a sigmoid output takes a handful of values, the 64
  // lanes of a wave serialise on one LDS word (17 K cycles even with one add per distinct digit of a
  // wave-instruction).  Any MONOTONE bucket function will do: bucket(key) = the score's exponent and top four
  // mantissa bits, v = key >> 51, as v - 1776 clamped to [0, 255] -- sixteen buckets per octave from 2^-16 up to 1;
  // bucket 0 (everything up to 2^-16) and bucket 255 (v >= 2031) are catch-alls.
  // A sweep over a thread's 12 keys costs ~2.5 K cycles however little it does (16 waves x 12 keys on 4 SIMDs), so
  // there are two: the one above (keys + bucket histogram) and ONE that files every key by its bucket -- above the
  // K-th key's bucket: selected; in it: a candidate (LDS list).  The byte passes then run over the candidates
  // only.  The keys of a bucket 1..254 share their top 12 bits: the byte passes continue below them; in a
  // catch-all they start from the top.
  unsigned long long prefix = 0, pmask = 0, floor_ = 0;
  int remaining = K, npass = 0, sh = 0;
  bool done;
  // every wave scans a histogram's 256 bins from the top down (lane l owns bins 255-4l .. 252-4l): the bin that
  // holds the remaining-th key, the keys above that bin, the bin's own count -- the same in every wave
  auto scan = [&](const unsigned int* hist, int& bin, int& cum, int& cnt) {
    const uint4 h4 = *reinterpret_cast<const uint4*>(&hist[252 - 4 * lane]);
    const int c0 = (int)h4.w, c1 = (int)h4.z, c2 = (int)h4.y, c3 = (int)h4.x;
    const int sum = c0 + c1 + c2 + c3;
    const int incl = wave_scan_incl(sum);
    const int excl = incl - sum;
    const bool mine = excl < remaining && remaining <= incl;      // exactly one lane
    cum = excl; bin = 255 - 4 * lane; cnt = c0;
    if (cum + c0 < remaining) { cum += c0; bin -= 1; cnt = c1;
      if (cum + c1 < remaining) { cum += c1; bin -= 1; cnt = c2;
        if (cum + c2 < remaining) { cum += c2; bin -= 1; cnt = c3; } } }
    const int owner = __builtin_ctzll(__ballot(mine));
    bin = __builtin_amdgcn_readlane(bin, owner); cum = __builtin_amdgcn_readlane(cum, owner);
    cnt = __builtin_amdgcn_readlane(cnt, owner);
  };
  const unsigned long long below = (1ull << lane) - 1ull;
  int fstar, cum, cnt;
  scan(S.hist[0], fstar, cum, cnt);
  remaining -= cum;
  // every key of the chosen bin is wanted: the lower digits cannot change the selection, the remaining
  // passes (normally those over the index half of the key, ties between scores being rare) are skipped
  done = remaining == cnt;
  floor_ = fstar == 0 ? 0ull : (unsigned long long)(fstar + 1776) << 51;         // the bucket's lower bound
  DEC_STAMP(3);
  {
    unsigned long long ms[DEC_NK], mc[DEC_NK];
    int ts = 0, tc_ = 0;
#pragma unroll
    for (int j = 0; j < DEC_NK; ++j) {
      const int bj = key[j] != 0ull ? (int)bucket(key[j]) : -1;
      ms[j] = __ballot(bj > fstar || (done && bj == fstar));
      mc[j] = __ballot(!done && bj == fstar);
      ts += __popcll(ms[j]); tc_ += __popcll(mc[j]);
    }
    unsigned bs = 0, bc = 0;
    if (lane == 0) {                                     // one atomic per list and wave
      if (ts) bs = atomicAdd(&S.count, (unsigned)ts);
      if (tc_) bc = atomicAdd(&S.ccount, (unsigned)tc_);
    }
    bs = (unsigned)__builtin_amdgcn_readfirstlane((int)bs); bc = (unsigned)__builtin_amdgcn_readfirstlane((int)bc);
#pragma unroll
    for (int j = 0; j < DEC_NK; ++j) {
      if ((ms[j] >> lane) & 1ull) { const unsigned pos = bs + (unsigned)__popcll(ms[j] & below); if (pos < DEC_MAXK) S.sel[pos] = key[j]; }
      if ((mc[j] >> lane) & 1ull) cand[bc + (unsigned)__popcll(mc[j] & below)] = key[j];
      bs += (unsigned)__popcll(ms[j]); bc += (unsigned)__popcll(mc[j]);
    }
  }
  DEC_STAMP(4);
  if (!done) {
    const bool normal = fstar >= 1 && fstar <= 254;
    prefix = normal ? floor_ : 0ull;
    pmask = normal ? 0xFFFull << 51 : 0ull;
    sh = normal ? 51 : 63;
    __syncthreads();
    const int ncand = (int)S.ccount;
#pragma unroll 1
    for (;;) {
      const int w = min(8, sh);                          // the last field is what is left: 3 or 7 bits
      sh -= w;
      const unsigned dmask = (1u << w) - 1u;
      unsigned int* hist = S.hist[++npass];
      for (int i = tid; i < ncand; i += DEC_THREADS) {
        const unsigned long long k = cand[i];
        if ((k & pmask) == prefix) atomicAdd(&hist[(unsigned)(k >> sh) & dmask], 1u);
      }
      pmask |= (unsigned long long)dmask << sh;
      __syncthreads();
      int bin;
      scan(hist, bin, cum, cnt);
      remaining -= cum;
      prefix |= (unsigned long long)(unsigned)bin << sh;
      DEC_STAMP(4 + npass);
      if (remaining == cnt || sh == 0) break;
    }
    // exactly `remaining` candidates are >= prefix (keys are unique; prefix has zeros below the digits examined;
    // in the upper catch-all an early exit can leave it below the bucket's floor -- the list holds the bucket only)
    for (int i0 = 0; i0 < ncand; i0 += DEC_THREADS) {
      const int i = i0 + tid;
      const unsigned long long k = i < ncand ? cand[i] : 0ull;
      const unsigned long long m = __ballot(k != 0ull && k >= prefix);
      if (m != 0ull) {
        unsigned base = 0;
        if (lane == 0) base = atomicAdd(&S.count, (unsigned)__popcll(m));
        base = (unsigned)__builtin_amdgcn_readfirstlane((int)base);
        const unsigned pos = base + (unsigned)__popcll(m & below);
        if (((m >> lane) & 1ull) && pos < DEC_MAXK) S.sel[pos] = k;
      }
    }
  }
  DEC_STAMP(11);
  __syncthreads();
  DEC_STAMP(12);
  // rank, descending: a survivor's place = the number of survivors above it.  A thread compares FOUR survivors
  // (registers) with one slice of the list (16-byte LDS reads: with one survivor per thread the 1024 threads
  // pulled 1.2 MB through the LDS port -- 10 K cycles) and adds its counts to the survivors' rank words.
  {
    const int kpad = (K + 3) & ~3;
    const int groups = kpad >> 2, parts = DEC_THREADS / groups;           // K = 300: 75 groups x 13 slices
    const int g = tid % groups, part = tid / groups;
    int chunk = (kpad + parts - 1) / parts;
    chunk = (chunk + 1) & ~1;
    if (part < parts) {
      const ulonglong2 a01 = *reinterpret_cast<const ulonglong2*>(&S.sel[4 * g]);
      const ulonglong2 a23 = *reinterpret_cast<const ulonglong2*>(&S.sel[4 * g + 2]);
      int r0 = 0, r1 = 0, r2 = 0, r3 = 0;
      const int j1 = min(kpad, (part + 1) * chunk);
      for (int j = part * chunk; j < j1; j += 2) {
        const ulonglong2 o = *reinterpret_cast<const ulonglong2*>(&S.sel[j]);
        r0 += (o.x > a01.x ? 1 : 0) + (o.y > a01.x ? 1 : 0);
        r1 += (o.x > a01.y ? 1 : 0) + (o.y > a01.y ? 1 : 0);
        r2 += (o.x > a23.x ? 1 : 0) + (o.y > a23.x ? 1 : 0);
        r3 += (o.x > a23.y ? 1 : 0) + (o.y > a23.y ? 1 : 0);
      }
      if (r0) atomicAdd(&S.rank[4 * g + 0], (unsigned)r0);
      if (r1) atomicAdd(&S.rank[4 * g + 1], (unsigned)r1);
      if (r2) atomicAdd(&S.rank[4 * g + 2], (unsigned)r2);
      if (r3) atomicAdd(&S.rank[4 * g + 3], (unsigned)r3);
    }
  }
  __syncthreads();
  DEC_STAMP(13);
  // thread t decodes survivor t into output row rank[t]; rows K .. max_num - 1 (fewer candidates than max_num): zeros
  // (max_num <= DEC_MAXK < DEC_THREADS: one survivor per thread at most)
  {
    const int t = tid;
    const bool row = t < p.K, have = t < K;
    const int i = have ? (int)S.rank[t] : t;
    float o[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float score = 0.f;
    int label = -1;
    bool ok = false;
    if (have) {
      const unsigned long long k = S.sel[t];
      const int idx = (int)(0xFFFFFFFFu - (unsigned int)(k & 0xFFFFFFFFull));
      score = __uint_as_float((unsigned int)(k >> 32));
      label = idx % p.ncls;
      const float* nb = p.box + ((size_t)b * p.Q + idx / p.ncls) * p.code;
      // UTIL:26-52
      const float rot = atan2f(nb[6], nb[7]);
      const float cx = nb[0], cy = nb[1], cz = nb[4];
      const float w = expf(nb[2]), l = expf(nb[3]), h = expf(nb[5]);
      ok = cx >= p.pcr[0] && cy >= p.pcr[1] && cz >= p.pcr[2] && cx <= p.pcr[3] && cy <= p.pcr[4] && cz <= p.pcr[5];
      o[0] = cx; o[1] = cy; o[2] = p.z_shift ? cz - h * 0.5f : cz;   // HEAD:1018
      o[3] = w; o[4] = l; o[5] = h; o[6] = rot;
      o[7] = p.code > 8 ? nb[8] : 0.f; o[8] = p.code > 9 ? nb[9] : 0.f;
    }
    if (row && p.boxes != nullptr) {
      float* ob = p.boxes + ((size_t)b * p.K + i) * 9;
#pragma unroll
      for (int j = 0; j < 9; ++j) ob[j] = o[j];
      p.scores[(size_t)b * p.K + i] = score; p.labels[(size_t)b * p.K + i] = label;
      p.valid[(size_t)b * p.K + i] = ok ? 1 : 0;
    }
    if (p.kboxes != nullptr) {                      // (uniform)
      // CODER:62-76: the range mask is taken on the coder's own (un-shifted) centre, the threshold is strict
      const bool kept = have && ok && (!p.use_thr || score > p.thr);
      if (kept) atomicOr(&S.keep[i >> 6], 1ull << (i & 63));
      __syncthreads();
      int below_words = 0, total = 0;
#pragma unroll
      for (int wd = 0; wd < DEC_MAXK / 64; ++wd) {
        const int c = __popcll(S.keep[wd]);
        total += c;
        if (wd < (i >> 6)) below_words += c;
      }
      if (kept) {
        const int pos = below_words + __popcll(S.keep[i >> 6] & ((1ull << (i & 63)) - 1ull));
        float* ob = p.kboxes + ((size_t)b * p.K + pos) * 9;
#pragma unroll
        for (int j = 0; j < 9; ++j) ob[j] = o[j];
        p.kscores[(size_t)b * p.K + pos] = score; p.klabels[(size_t)b * p.K + pos] = (long long)label;
      }
      if (tid == 0) p.kcount[b] = total;
    }
  }
  DEC_STAMP(14);
}

#ifdef TC_CHAIN_STAMPS
extern "C" int tc_debug_decode_stamps(long long* host_out) {
  return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_dec_stamps), sizeof(long long) * 16);
}
#endif

// ---- the streaming kernel: any Q * num_classes up to DEC_STREAM_MAXN, max_num up to DEC_STREAM_MAXK ----------------------
// The same key, the same select (bucket pass, then byte passes inside the chosen bucket, ties to the lower flat index)
// and the same outputs as box_decode_kernel, for the shapes its registers and its one-survivor-per-thread stages cannot
// take.  Nothing of a key is kept: every pass reads the sample's logits again (a few hundred KB at most: L2) and
// rebuilds the key -- sigmoidf_ is deterministic, so the bits are those of the pass before.  There is no candidate
// list, so no overflow route either: a byte pass counts the keys of the chosen bucket that match the digits fixed so
// far.  Behind the select every stage strides over its rows by the workgroup size.
// Every loop around a barrier or a ballot runs a workgroup-uniform number of times: the stream loops go from 0 to n in
// steps of the workgroup size whatever the thread (the tail is masked, not skipped), and the byte-pass loop leaves on
// values every wave reads from the same histogram behind the same barrier.
constexpr int DEC_STREAM_MAXN = TC_BOX_DECODE_STREAM_MAX_SCORES;    // the index math stays in 32 bits
constexpr int DEC_STREAM_MAXK = TC_BOX_DECODE_STREAM_MAX_NUM;
static_assert(DEC_MAXN == TC_BOX_DECODE_MAX_SCORES && DEC_MAXK == TC_BOX_DECODE_MAX_NUM, "the header's in-register caps");
static_assert(DEC_STREAM_MAXK % 64 == 0 && DEC_STREAM_MAXK % DEC_THREADS == 0, "whole keep words, whole strides");

struct DecStreamLds {
  alignas(16) unsigned int hist[DEC_PASSES][256];
  alignas(16) unsigned long long sel[DEC_STREAM_MAXK];   // survivors: any order, then descending; zero behind them
  unsigned int rank[DEC_STREAM_MAXK];                    // survivor -> its place in descending order
  unsigned long long keep[DEC_STREAM_MAXK / 64];         // bit i: output row i is kept
  unsigned int count;
};

__device__ __forceinline__ unsigned long long dec_key(float logit, int i) {
  return ((unsigned long long)__float_as_uint(sigmoidf_(logit)) << 32) | (unsigned int)(0xFFFFFFFFu - (unsigned)i);
}

__global__ __launch_bounds__(DEC_THREADS) void box_decode_stream_kernel(DecK p) {
  __shared__ DecStreamLds S;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int n = p.Q * p.ncls;
  const float* cls = p.cls + (size_t)b * n;            // n odd: 4-byte aligned only -- one float per load
  for (int i = tid; i < DEC_PASSES * 256; i += DEC_THREADS) (&S.hist[0][0])[i] = 0u;
  for (int i = tid; i < DEC_STREAM_MAXK; i += DEC_THREADS) { S.sel[i] = 0ull; S.rank[i] = 0u; }
  if (tid < DEC_STREAM_MAXK / 64) S.keep[tid] = 0ull;
  if (tid == 0) S.count = 0u;
  __syncthreads();
  // one add per key; a wave-instruction whose keys all fall into ONE bin (equal scores, a catch-all, the upper index
  // digits of neighbouring keys) adds their number once instead of serialising 64 lanes on the word
  auto count_digit = [&](unsigned int* hist, bool match, unsigned d) {
    const unsigned long long m = __ballot(match);
    if (m != 0ull) {                                     // (wave-uniform)
      const int first = __builtin_ctzll(m);
      const unsigned d0 = (unsigned)__builtin_amdgcn_readlane((int)d, first);
      if (__ballot(match && d != d0) == 0ull) {
        if (lane == first) atomicAdd(&hist[d0], (unsigned)__popcll(m));
      } else if (match) {
        atomicAdd(&hist[d], 1u);
      }
    }
  };
  for (int i0 = 0; i0 < n; i0 += DEC_THREADS) {
    const int i = i0 + tid;
    const bool act = i < n;
    const unsigned long long k = act ? dec_key(cls[i], i) : 0ull;
    count_digit(S.hist[0], act, bucket(k));
  }
  __syncthreads();
  const int K = min(p.K, n);
  // the scan of box_decode_kernel: the bin that holds the remaining-th key from the top, the keys above that bin, the
  // bin's own count -- every wave for itself, the same in every wave
  int remaining = K;
  auto scan = [&](const unsigned int* hist, int& bin, int& cum, int& cnt) {
    const uint4 h4 = *reinterpret_cast<const uint4*>(&hist[252 - 4 * lane]);
    const int c0 = (int)h4.w, c1 = (int)h4.z, c2 = (int)h4.y, c3 = (int)h4.x;
    const int sum = c0 + c1 + c2 + c3;
    const int incl = wave_scan_incl(sum);
    const int excl = incl - sum;
    const bool mine = excl < remaining && remaining <= incl;      // exactly one lane (1 <= remaining <= the keys counted)
    cum = excl; bin = 255 - 4 * lane; cnt = c0;
    if (cum + c0 < remaining) { cum += c0; bin -= 1; cnt = c1;
      if (cum + c1 < remaining) { cum += c1; bin -= 1; cnt = c2;
        if (cum + c2 < remaining) { cum += c2; bin -= 1; cnt = c3; } } }
    const int owner = __builtin_ctzll(__ballot(mine));
    bin = __builtin_amdgcn_readlane(bin, owner); cum = __builtin_amdgcn_readlane(cum, owner);
    cnt = __builtin_amdgcn_readlane(cnt, owner);
  };
  int fstar, cum, cnt;
  scan(S.hist[0], fstar, cum, cnt);
  remaining -= cum;
  const bool done = remaining == cnt;                    // the whole bucket is wanted (K = n ends here at the latest)
  // the K-th key's digits below the bucket: a key of bucket 1..254 shares its top 12 bits with the bucket, the byte
  // passes go on below them; in a catch-all they start from the top.  prefix keeps zeros below the digits examined
  unsigned long long prefix = 0ull, pmask = 0ull;
  if (!done) {
    const bool normal = fstar >= 1 && fstar <= 254;
    prefix = normal ? (unsigned long long)(fstar + 1776) << 51 : 0ull;
    pmask = normal ? 0xFFFull << 51 : 0ull;
    int sh = normal ? 51 : 63, npass = 0;
#pragma unroll 1
    for (;;) {                                           // at most eight times: 63 = 7 x 8 + 7 bits, 51 = 6 x 8 + 3
      const int w = min(8, sh);
      sh -= w;
      const unsigned dmask = (1u << w) - 1u;
      unsigned int* hist = S.hist[++npass];
      for (int i0 = 0; i0 < n; i0 += DEC_THREADS) {
        const int i = i0 + tid;
        const bool act = i < n;
        const unsigned long long k = act ? dec_key(cls[i], i) : 0ull;
        count_digit(hist, act && (int)bucket(k) == fstar && (k & pmask) == prefix, (unsigned)(k >> sh) & dmask);
      }
      pmask |= (unsigned long long)dmask << sh;
      __syncthreads();
      int bin;
      scan(hist, bin, cum, cnt);
      remaining -= cum;
      prefix |= (unsigned long long)(unsigned)bin << sh;
      if (remaining == cnt || sh == 0) break;            // (read from LDS behind the barrier: the same in every wave)
    }
  }
  // the survivors: everything above the bucket, and of the bucket the keys >= prefix (done: prefix = 0, all of it) --
  // exactly K keys, one atomic per wave-instruction
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int i0 = 0; i0 < n; i0 += DEC_THREADS) {
    const int i = i0 + tid;
    const bool act = i < n;
    const unsigned long long k = act ? dec_key(cls[i], i) : 0ull;
    const int bk = (int)bucket(k);
    const unsigned long long m = __ballot(act && (bk > fstar || (bk == fstar && k >= prefix)));
    if (m != 0ull) {                                     // (wave-uniform)
      unsigned base = 0;
      if (lane == 0) base = atomicAdd(&S.count, (unsigned)__popcll(m));
      base = (unsigned)__builtin_amdgcn_readfirstlane((int)base);
      const unsigned pos = base + (unsigned)__popcll(m & below);
      if (((m >> lane) & 1ull) && pos < (unsigned)DEC_STREAM_MAXK) S.sel[pos] = k;
    }
  }
  __syncthreads();
  // rank, descending: a survivor's place = the number of survivors above it (keys are unique, the zeros behind the
  // K-th are above nothing).  K <= 1024: a survivor's K compares are split over 1024 / K threads.  At most K * K = 4 M
  // compares; the reads of a wave are one address or neighbours.
  {
    const int parts = max(1, DEC_THREADS / K);
    const int chunk = (K + parts - 1) / parts;
    for (int w = tid; w < K * parts; w += DEC_THREADS) {
      const int t = w % K, part = w / K;
      const unsigned long long a = S.sel[t];
      const int j1 = min(K, (part + 1) * chunk);
      int r = 0;
      for (int j = part * chunk; j < j1; ++j) r += S.sel[j] > a ? 1 : 0;
      if (r) atomicAdd(&S.rank[t], (unsigned)r);
    }
  }
  __syncthreads();
  // into descending order, in place: through registers, a barrier between the reads and the writes
  {
    unsigned long long kk[DEC_STREAM_MAXK / DEC_THREADS];
    unsigned int rk[DEC_STREAM_MAXK / DEC_THREADS];
#pragma unroll
    for (int r = 0; r < DEC_STREAM_MAXK / DEC_THREADS; ++r) {
      const int t = tid + r * DEC_THREADS;
      kk[r] = t < K ? S.sel[t] : 0ull; rk[r] = t < K ? S.rank[t] : 0u;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < DEC_STREAM_MAXK / DEC_THREADS; ++r)
      if (tid + r * DEC_THREADS < K && rk[r] < (unsigned)DEC_STREAM_MAXK) S.sel[rk[r]] = kk[r];
    __syncthreads();
  }
  // output row i < K decodes survivor i; rows K .. max_num - 1 (fewer candidates than max_num): zeros, label -1
  struct Row { float o[9]; float score; int label; bool ok; };
  auto decode = [&](int i) {
    Row r;
#pragma unroll
    for (int j = 0; j < 9; ++j) r.o[j] = 0.f;
    r.score = 0.f; r.label = -1; r.ok = false;
    if (i < K) {
      const unsigned long long k = S.sel[i];
      const int idx = (int)(0xFFFFFFFFu - (unsigned int)(k & 0xFFFFFFFFull));
      r.score = __uint_as_float((unsigned int)(k >> 32));
      r.label = idx % p.ncls;
      const float* nb = p.box + ((size_t)b * p.Q + idx / p.ncls) * p.code;
      // UTIL:26-52
      const float rot = atan2f(nb[6], nb[7]);
      const float cx = nb[0], cy = nb[1], cz = nb[4];
      const float w = expf(nb[2]), l = expf(nb[3]), h = expf(nb[5]);
      r.ok = cx >= p.pcr[0] && cy >= p.pcr[1] && cz >= p.pcr[2] && cx <= p.pcr[3] && cy <= p.pcr[4] && cz <= p.pcr[5];
      r.o[0] = cx; r.o[1] = cy; r.o[2] = p.z_shift ? cz - h * 0.5f : cz;   // HEAD:1018
      r.o[3] = w; r.o[4] = l; r.o[5] = h; r.o[6] = rot;
      r.o[7] = p.code > 8 ? nb[8] : 0.f; r.o[8] = p.code > 9 ? nb[9] : 0.f;
    }
    return r;
  };
  for (int i = tid; i < p.K; i += DEC_THREADS) {
    const Row r = decode(i);
    if (p.boxes != nullptr) {
      float* ob = p.boxes + ((size_t)b * p.K + i) * 9;
#pragma unroll
      for (int j = 0; j < 9; ++j) ob[j] = r.o[j];
      p.scores[(size_t)b * p.K + i] = r.score; p.labels[(size_t)b * p.K + i] = r.label;
      p.valid[(size_t)b * p.K + i] = r.ok ? 1 : 0;
    }
    // CODER:62-76: the range mask is taken on the coder's own (un-shifted) centre, the threshold is strict
    if (p.kboxes != nullptr && r.ok && (!p.use_thr || r.score > p.thr)) atomicOr(&S.keep[i >> 6], 1ull << (i & 63));
  }
  if (p.kboxes != nullptr) {                          // (uniform: a kernel argument)
    __syncthreads();
    for (int i = tid; i < K; i += DEC_THREADS) {
      if (!((S.keep[i >> 6] >> (i & 63)) & 1ull)) continue;
      int pos = __popcll(S.keep[i >> 6] & ((1ull << (i & 63)) - 1ull));
      for (int wd = 0; wd < (i >> 6); ++wd) pos += __popcll(S.keep[wd]);
      const Row r = decode(i);
      float* ob = p.kboxes + ((size_t)b * p.K + pos) * 9;
#pragma unroll
      for (int j = 0; j < 9; ++j) ob[j] = r.o[j];
      p.kscores[(size_t)b * p.K + pos] = r.score; p.klabels[(size_t)b * p.K + pos] = (long long)r.label;
    }
    if (tid == 0) {
      int total = 0;
      for (int wd = 0; wd < DEC_STREAM_MAXK / 64; ++wd) total += __popcll(S.keep[wd]);
      p.kcount[b] = total;
    }
  }
}

size_t box_decode_ws_bytes(int, int, int) { return 256; }

int launch_box_decode(const float* cls, const float* box, int B, int Q, int ncls, int code,
                      int max_num, const float* pcr6_host, float* boxes, float* scores, int* labels,
                      unsigned char* valid, void*, size_t, hipStream_t s, const BoxDecodeKept* kept, int path) {
  // (64-bit: Q * num_classes itself may not fit an int)
  const long long n64 = (long long)Q * (long long)ncls;
  TC_REQUIRE(B >= 1 && Q >= 1 && ncls >= 1, "box_decode: B=%d, Q=%d, num_classes=%d", B, Q, ncls);
  TC_REQUIRE(path >= 0 && path <= 2, "box_decode: path=%d (0 automatic, 1 in-register, 2 streaming)", path);
  TC_REQUIRE(n64 <= DEC_STREAM_MAXN, "box_decode: Q*num_classes=%lld > %d", n64, DEC_STREAM_MAXN);
  TC_REQUIRE(max_num >= 1 && max_num <= DEC_STREAM_MAXK, "box_decode: max_num=%d (1..%d)", max_num, DEC_STREAM_MAXK);
  const bool fits = n64 <= DEC_MAXN && max_num <= DEC_MAXK;
  if (path == 1) {
    TC_REQUIRE(n64 <= DEC_MAXN, "box_decode: Q*num_classes=%lld > %d, the in-register kernel's (path 1)", n64, DEC_MAXN);
    TC_REQUIRE(max_num <= DEC_MAXK, "box_decode: max_num=%d > %d, the in-register kernel's (path 1)", max_num, DEC_MAXK);
  }
  const bool stream = path == 2 || !fits;
  TC_REQUIRE(code >= 8, "box_decode: code_size=%d", code);
  // a call whose pointers are missing is refused here and not by a fault in the kernel; the message carries the call's
  // shape (the callers that probe the entries hand in no pointers at all)
#define DEC_REQUIRE_PTR(cond, what)                                                                                 \
  TC_REQUIRE(cond, "box_decode: " what " (B=%d, Q=%d, num_classes=%d, code_size=%d, max_num=%d)", B, Q, ncls, code, max_num)
  DEC_REQUIRE_PTR(boxes != nullptr || kept != nullptr, "no output");
  DEC_REQUIRE_PTR(boxes == nullptr || (scores != nullptr && labels != nullptr && valid != nullptr),
                  "fixed-size outputs come together");
  DEC_REQUIRE_PTR(kept == nullptr || (kept->boxes && kept->scores && kept->labels && kept->count),
                  "kept outputs come together");
  DEC_REQUIRE_PTR(cls != nullptr && box != nullptr && pcr6_host != nullptr, "null cls_scores, bbox_preds or post_center_range");
#undef DEC_REQUIRE_PTR
  DecK p;
  p.cls = cls; p.box = box; p.Q = Q; p.ncls = ncls; p.code = code; p.K = max_num;
  for (int i = 0; i < 6; ++i) p.pcr[i] = pcr6_host[i];
  p.boxes = boxes; p.scores = scores; p.labels = labels; p.valid = valid;
  p.kboxes = nullptr; p.kscores = nullptr; p.klabels = nullptr; p.kcount = nullptr; p.thr = 0.f; p.use_thr = 0; p.z_shift = 1;
  if (kept != nullptr) {
    p.kboxes = kept->boxes; p.kscores = kept->scores; p.klabels = kept->labels; p.kcount = kept->count;
    p.thr = kept->score_threshold; p.use_thr = kept->use_threshold; p.z_shift = kept->z_shift;
  }
  if (stream) {
    hipLaunchKernelGGL(box_decode_stream_kernel, dim3(B), dim3(DEC_THREADS), 0, s, p);
    return check_launch("box_decode(stream)");
  }
  const size_t lds = (size_t)((Q * ncls + 1) & ~1) * 8;
  static DeviceOnce once;
  if (const int once_dev = once.need(); once_dev >= 0) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(box_decode_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, DEC_MAXN * 8);
    if (e != hipSuccess) { set_error("box_decode: %s", hipGetErrorString(e)); return (int)e; }
    once.done(once_dev);
  }
  hipLaunchKernelGGL(box_decode_kernel, dim3(B), dim3(DEC_THREADS), lds, s, p);
  return check_launch("box_decode");
}

}  // namespace tc
