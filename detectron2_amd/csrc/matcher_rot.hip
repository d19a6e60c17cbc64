// Fused ROTATED anchor matching: pairwise_iou_rotated + Matcher without the M x N matrix.
//   replaces  detectron2/structures/rotated_boxes.py:483-503 (pairwise_iou_rotated) followed by
//             detectron2/modeling/matcher.py:62-127 (Matcher.__call__, set_low_quality_matches_)
//   as called from proposal_generator/rrpn.py:151-200 (G x 268,569 rotated anchors per image, one image at a time).
// The reference writes the matrix (17 MB per image), more than 99 % of it exact zeros (rot_pair_is_zero, rotated_iou.h),
// and makes ~8 passes over it.  Here a WORKGROUP (MR_STRIP = 128 threads) OWNS A STRIP of 128 boxes of one image:
//   1. a chunk of MR_CHUNK = 64 ground-truth boxes of the image goes to LDS; lane b runs the exact zero test of box b
//      against each of them (64 bits of "needs the clip" per lane).  A zero takes part in the column maximum from a
//      register (the first zero index is all that matters) and in the row maximum through one ballot per wave: no store;
//   2. the survivors are appended to an LDS list of MR_LIST (gt << 7 | box) entries -- wave prefix, one LDS counter add
//      per wave.  What does not fit stays in the lane's bit mask;
//   3. the list is DRAINED: lane = one listed pair runs the polygon clip (single_box_iou_rotated, b1 = ground truth,
//      b2 = box).  Pairs finish in list order, so the column maximum is a 64-bit LDS atomicMax on
//      (ordered IoU key << 32 | ~ground-truth index): the larger value wins, among equals the LOWER index -- torch.max's
//      rule.  Steps 2-3 repeat while any lane has bits left: a strip whose 128 x 64 pairs all survive (every box on one
//      spot) takes 8 drains; nothing is sized for the worst case.
// Row maxima (allow_low_quality_matches only): LDS atomicMax per surviving pair, then one global atomicMax per workgroup
// and ground-truth box.  The low-quality pass is a second launch of the same skeleton that RECOMPUTES survivors' values
// (the same function on the same inputs: the same bits) and compares keys with the row maxima -- but only for the pairs
// of a box whose own column maximum (4 bytes per box kept by the first launch) reaches the row's maximum: no other pair
// can equal it.  A ground-truth box that overlaps nothing has row maximum 0 and marks every box with quality 0, like
// the reference's `==` + nonzero.
// LDS per workgroup: 24 KB clip scratch + 2.5 KB boxes + 1.25 KB ground truth + 2 KB list + 1 KB column keys.
// Bit-exact for finite boxes (this unit is compiled with -ffp-contract=off, like iou.hip).  Non-finite coordinates are
// outside the contract; every LDS index comes from lane and list positions, never from a coordinate, and the clip's
// point count is bounded by its loop structure (16 + 4 + 4), so they cannot index outside LDS.
#pragma clang fp contract(off)
#include "common.h"
#include "matcher_core.h"
#include "rotated_iou.h"

namespace d2amd {

constexpr int MR_STRIP = 128;       // boxes per workgroup == threads
constexpr int MR_CHUNK = 64;        // ground-truth boxes staged per LDS pass (one bit each in a lane's mask)
constexpr int MR_LIST = 1024;       // capacity of the survivor list
constexpr int MR_MAX_IMAGES = 16;   // images per launch (blockIdx.y)

// order-preserving float -> uint key for ANY value (a degenerate tiny box can give a negative or infinite quotient);
// -0 and +0 share a key (torch compares them equal), NaN maps above every number like torch.max
__device__ __forceinline__ uint32_t mr_key(float v) {
  if (v != v) return 0xffffffffu;
  if (v == 0.f) return 0x80000000u;
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float mr_unkey(uint32_t k) {
  if (k == 0xffffffffu) return __builtin_nanf("");
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
constexpr uint32_t MR_KEY_ZERO = 0x80000000u;

struct MrBatch {
  const float* gt[MR_MAX_IMAGES];
  int M[MR_MAX_IMAGES];
  long out_stride;  // elements between the images' rows of matches / labels
  int rm_stride;    // words between the images' row maxima
};
// (constant indices only into the kernel-argument struct: a dynamic one makes the compiler copy it to scratch)
__device__ __forceinline__ void mr_image(const MrBatch& B, int img, const float*& gt, int& M) {
  gt = B.gt[0]; M = B.M[0];
#pragma unroll
  for (int q = 1; q < MR_MAX_IMAGES; q++)
    if (q == img) { gt = B.gt[q]; M = B.M[q]; }
}

// LOWQ false: column maxima -> matches / labels (and the row maxima when rowmax != nullptr)
// LOWQ true:  set_low_quality_matches_ from the finished row maxima
template <bool LOWQ>
__global__ __launch_bounds__(MR_STRIP) void match_rotated_kernel(const MrBatch B, const float* __restrict__ boxes, int N,
                                                                 MatchCfg cfg, int64_t* __restrict__ matches,
                                                                 int8_t* __restrict__ labels,
                                                                 uint32_t* __restrict__ rowmax,
                                                                 uint32_t* __restrict__ colkey) {
  const float* gt;
  int M;
  mr_image(B, blockIdx.y, gt, M);
  if (!LOWQ) matches += (long)blockIdx.y * B.out_stride;
  labels += (long)blockIdx.y * B.out_stride;
  if (rowmax) rowmax += (long)blockIdx.y * B.rm_stride;
  if (colkey) colkey += (long)blockIdx.y * B.out_stride;

  __shared__ RotIouScratch<MR_STRIP> S;
  __shared__ float s_box[5][MR_STRIP];
  __shared__ float s_gt[MR_CHUNK][5];
  __shared__ uint32_t s_rmax[MR_CHUNK];              // !LOWQ: the chunk's row maxima of this strip; LOWQ: the final ones
  __shared__ unsigned long long s_cmax[MR_STRIP];    // !LOWQ: key << 32 | ~index
  __shared__ int s_hit[MR_STRIP];                    // LOWQ
  __shared__ uint16_t s_list[MR_LIST];
  __shared__ int s_n;
  __shared__ MatchCfg s_cfg;  // (13 scalar registers held to the end otherwise: the clip's nested branches need them)

  const int tid = threadIdx.x, lane = tid & 63;
  const long n = (long)blockIdx.x * MR_STRIP + tid;
  const bool valid = n < N;
  float cb[5];
#pragma unroll
  for (int k = 0; k < 5; k++) {
    cb[k] = boxes[(valid ? n : (long)N - 1) * 5 + k];
    s_box[k][tid] = cb[k];
  }
  s_cmax[tid] = 0ull;
  s_hit[tid] = 0;
  if (tid == 0) { s_n = 0; s_cfg = cfg; }
  int zfirst = -1;     // !LOWQ: first ground-truth index whose IoU with this box is an exact zero
  // LOWQ: the key of this box's column maximum.  A pair below it cannot equal a row maximum above it: only the pairs
  // of a box whose best quality reaches the row's maximum are clipped again (a few per ground-truth box)
  const uint32_t ckey = (LOWQ && valid) ? colkey[n] : 0u;
  bool hit = false;    // LOWQ

  for (int m0 = 0; m0 < M; m0 += MR_CHUNK) {
    const int mc = min(MR_CHUNK, M - m0);
    __syncthreads();  // (the previous chunk's drains are over)
    for (int i = tid; i < mc * 5; i += MR_STRIP) s_gt[i / 5][i % 5] = gt[(long)m0 * 5 + i];
    if (tid < mc) s_rmax[tid] = LOWQ ? rowmax[m0 + tid] : 0u;
    __syncthreads();

    // 1. the exact zero test of this lane's box against the chunk
    unsigned long long live = 0ull;
    for (int i = 0; i < mc; i++) {
      float gb[5];
#pragma unroll
      for (int k = 0; k < 5; k++) gb[k] = s_gt[i][k];
      const bool zero = valid && rot_pair_is_zero(gb, cb);
      if (LOWQ) {
        if (valid && !zero && ckey >= s_rmax[i]) live |= 1ull << i;
        if (zero && s_rmax[i] == MR_KEY_ZERO) hit = true;
      } else {
        if (valid && !zero) live |= 1ull << i;
        if (zero && zfirst < 0) zfirst = m0 + i;
        if (rowmax != nullptr && __ballot(zero) != 0ull && lane == 0) atomicMax(&s_rmax[i], MR_KEY_ZERO);
      }
    }

    // 2 + 3. append what fits, drain, until no lane has a pair left
    for (;;) {
      const int mine = __popcll(live);
      int incl = mine;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(incl, d, 64);
        if (lane >= d) incl += y;
      }
      const int total = __shfl(incl, 63, 64);
      int base = 0;
      if (lane == 63 && total > 0) base = atomicAdd(&s_n, total);
      base = __shfl(base, 63, 64);
      int at = base + incl - mine;
      while (live != 0ull && at < MR_LIST) {
        const int i = __builtin_ctzll(live);
        live &= live - 1ull;
        s_list[at++] = (uint16_t)((i << 7) | tid);
      }
      const int pending = __syncthreads_or(live != 0ull);  // (also: the list and s_n are complete)
      const int cnt = min(s_n, MR_LIST);
      for (int t0 = 0; t0 < cnt; t0 += MR_STRIP) {  // uniform
        const int t = t0 + tid;
        if (t < cnt) {
          const int e = s_list[t];
          const int i = e >> 7, c = e & (MR_STRIP - 1);
          float gb[5], bb[5];
#pragma unroll
          for (int k = 0; k < 5; k++) { gb[k] = s_gt[i][k]; bb[k] = s_box[k][c]; }
          const float v = single_box_iou_rotated<MR_STRIP>(gb, bb, S, tid);
          const uint32_t key = mr_key(v);
          if (LOWQ) {
            // float equality like the reference: NaN never equal, -0 == +0
            if (v == v && key == s_rmax[i]) s_hit[c] = 1;
          } else {
            atomicMax(&s_cmax[c], ((unsigned long long)key << 32) | (uint32_t)~(uint32_t)(m0 + i));
            if (rowmax != nullptr) atomicMax(&s_rmax[i], key);
          }
        }
      }
      __syncthreads();
      if (tid == 0) s_n = 0;
      if (!pending) break;  // uniform
      __syncthreads();
    }
    if (!LOWQ && rowmax != nullptr) {
      __syncthreads();
      // (a zero is a row's maximum candidate in every strip: without the read, 67,000 atomics on 32 addresses at the RRPN
      // shape.  The value only grows, so a stale read costs at most one atomic too many)
      if (tid < mc && s_rmax[tid] > __hip_atomic_load(&rowmax[m0 + tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        atomicMax(&rowmax[m0 + tid], s_rmax[tid]);
    }
  }
  __syncthreads();
  if (!valid) return;
  if (LOWQ) {
    if (hit || s_hit[tid] != 0) labels[n] = 1;
  } else {
    // torch.max(dim=0): first maximal value.  No ground truth: index 0, quality 0 (matcher.py:80-90: labels[0])
    unsigned long long best = s_cmax[tid];
    if (zfirst >= 0) {
      const unsigned long long z = ((unsigned long long)MR_KEY_ZERO << 32) | (uint32_t)~(uint32_t)zfirst;
      best = z > best ? z : best;
    }
    const bool none = best == 0ull;
    matches[n] = none ? 0 : (int64_t)(uint32_t)~(uint32_t)(best & 0xffffffffull);
    labels[n] = mt_label(none ? 0.f : mr_unkey((uint32_t)(best >> 32)), s_cfg);
    if (colkey) colkey[n] = none ? MR_KEY_ZERO : (uint32_t)(best >> 32);
  }
}

static int mr_cfg(const float* thresholds, const int8_t* labels, int T, MatchCfg& cfg) {
  D2_CHECK_ARG(T >= 0 && T <= D2AMD_MATCHER_MAX_THRESHOLDS && labels != nullptr && (T == 0 || thresholds != nullptr),
               "match_boxes_rotated: %d thresholds (max %d)", T, D2AMD_MATCHER_MAX_THRESHOLDS);
  cfg = MatchCfg{};
  cfg.T = T;
  for (int k = 0; k < T; k++) {
    D2_CHECK_ARG(thresholds[k] > 0.f && (k == 0 || thresholds[k - 1] <= thresholds[k]),
                 "match_boxes_rotated: thresholds must be positive and ascending");
    cfg.thr[k] = thresholds[k];
  }
  for (int k = 0; k <= T; k++) {
    D2_CHECK_ARG(labels[k] >= -1 && labels[k] <= 1, "match_boxes_rotated: labels must be in {-1, 0, 1}");
    cfg.lab[k] = labels[k];
  }
  return D2AMD_OK;
}

}  // namespace d2amd

using namespace d2amd;

// row maxima [count][rm_stride], then the boxes' column-maximum keys [count][N]
static size_t mr_rowmax_bytes(const int* M, int count) {
  int mmax = 1;
  for (int i = 0; i < count; i++) mmax = (M && M[i] > mmax) ? M[i] : mmax;
  return (size_t)(count > 0 ? count : 1) * ((mmax + 63) / 64 * 64) * 4;
}

extern "C" size_t d2amd_match_boxes_rotated_batch_workspace_bytes(const int* M, int count, int N) {
  return mr_rowmax_bytes(M, count) + (size_t)(count > 0 ? count : 0) * (size_t)(N > 0 ? N : 0) * 4;
}

extern "C" int d2amd_match_boxes_rotated_batch(const float* const* gt_boxes, const int* M, int count, const float* boxes,
                                               int N, const float* thresholds, const int8_t* labels, int T,
                                               int allow_low_quality, int64_t* matches, int8_t* match_labels,
                                               void* workspace, size_t workspace_bytes, void* stream) {
  const char* op = "match_boxes_rotated";
  D2_CHECK_ARG(count >= 0 && N >= 0, "%s: negative size", op);
  D2_CHECK_ARG(count == 0 || (gt_boxes != nullptr && M != nullptr), "%s: null image list", op);
  MatchCfg cfg;
  { const int rc = mr_cfg(thresholds, labels, T, cfg); if (rc) return rc; }
  int mmax = 0;
  for (int i = 0; i < count; i++) {
    D2_CHECK_ARG(M[i] >= 0, "%s: negative size", op);
    D2_CHECK_ARG(M[i] == 0 || gt_boxes[i] != nullptr, "%s: null ground truth of image %d", op, i);
    mmax = M[i] > mmax ? M[i] : mmax;
  }
  if (N == 0 || count == 0) return D2AMD_OK;
  D2_CHECK_ARG(boxes && matches && match_labels, "%s: null pointer", op);
  hipStream_t s = (hipStream_t)stream;
  const int rm_stride = (mmax + 63) / 64 * 64;
  uint32_t* rowmax = nullptr;
  uint32_t* colkey = nullptr;
  if (allow_low_quality && mmax > 0) {
    const size_t need = d2amd_match_boxes_rotated_batch_workspace_bytes(M, count, N);
    D2_CHECK_ARG(workspace != nullptr && ((uintptr_t)workspace & 15) == 0 && workspace_bytes >= need,
                 "%s: workspace missing, not 16-byte aligned or too small (%zu bytes, %zu needed)", op, workspace_bytes, need);
    rowmax = (uint32_t*)workspace;
    colkey = rowmax + mr_rowmax_bytes(M, count) / 4;
    { const int zrc = zero_async(rowmax, mr_rowmax_bytes(M, count), s); if (zrc) return zrc; }
  }
  const int grid = cdiv(N, MR_STRIP);
  for (int i0 = 0; i0 < count; i0 += MR_MAX_IMAGES) {
    const int c = count - i0 < MR_MAX_IMAGES ? count - i0 : MR_MAX_IMAGES;
    MrBatch Bt{};
    for (int i = 0; i < c; i++) { Bt.gt[i] = gt_boxes[i0 + i]; Bt.M[i] = M[i0 + i]; }
    Bt.out_stride = N;
    Bt.rm_stride = rm_stride;
    int64_t* mo = matches + (long)i0 * N;
    int8_t* lo = match_labels + (long)i0 * N;
    uint32_t* rm = rowmax ? rowmax + (long)i0 * rm_stride : nullptr;
    uint32_t* ck = colkey ? colkey + (long)i0 * N : nullptr;
    const bool timed = timing_begin("match_rotated", s);
    hipLaunchKernelGGL((match_rotated_kernel<false>), dim3(grid, c), dim3(MR_STRIP), 0, s, Bt, boxes, N, cfg, mo, lo, rm, ck);
    if (timed) timing_end("match_rotated", s);
    D2_LAUNCH_OK();
    if (rm) {
      hipLaunchKernelGGL((match_rotated_kernel<true>), dim3(grid, c), dim3(MR_STRIP), 0, s, Bt, boxes, N, cfg, nullptr, lo, rm, ck);
      D2_LAUNCH_OK();
    }
  }
  return D2AMD_OK;
}
