// Panoptic FPN merge: combine_semantic_and_instance_outputs (modeling/meta_arch/panoptic_fpn.py:184-269) on the device.
// The reference walks the detections in score order on the host -- per detection three .item() reads and about six
// full-image elementwise launches, then torch.unique(...).cpu() and one more read per stuff class.  Every quantity it
// compares is a pixel count, and a pixel's fate depends only on WHICH detections cover it and on its label.  So the image
// is reduced once to counted keys (128-bit set of covering ranks, label), and the greedy pass runs on those keys inside
// one workgroup.  Nothing is read on the host, nothing waits on another workgroup (no grid barrier, no flag).
//
// Launches on the caller's stream, one image per call:
//   rank      one workgroup of 128 threads: rank-by-counting of the <= 128 scores (descending, ties by lower index, the
//             candidates are those with (double)score >= instances_score_thresh) and the clearing of the counters.
//   coverage  one workgroup per 64 x 16 pixel tile, a thread per 4 consecutive pixels of a row (a wave = 4 rows of 64).
//             The set of a pixel lives in four registers, indexed statically.  Two mask sources:
//               pasted  (R, H, W) bytes: the candidates' rows in rank order, 4 B per thread and candidate: R_cand bytes
//                       per pixel read once (107 MB at 100 x 800 x 1333: the 107 MB the paste has just written).
//               fused   (R, M, M) soft masks + boxes: the rank-ordered list of candidates whose paste region meets the
//                       tile is built in LDS, their masks staged through LDS as fp32 in batches of floor(8192 / M^2),
//                       and the paste sample is evaluated per pixel inside the region -- the fp32 operation order and the
//                       region rule of paste_region_kernel (paste_masks.hip), so a bit is set exactly where
//                       paste_masks_in_image says so.  No (R, H, W) mask exists: R M^2 elements in, per tile.
//             Out: ceil(R / 32) set words per pixel (4 B each), the tile's label histogram (LDS, then <= 257 integer
//             atomics), and for COVERED pixels (set, label, count) records of 24 B: equal neighbours inside a thread are
//             merged, threads of one key along a wave's row are merged with DPP row_shr + ballot, the wave takes its slots
//             with one LDS atomic and the workgroup appends with ONE global atomic.  At most one record per covered pixel
//             (the workspace bound); integer sums, so the order of the records does not show in any output.
//   greedy    one workgroup of 1024 threads.  (1) the records -> distinct keys in an LDS table of 2048 slots: a slot is
//             claimed by atomicCAS of the claimant's RECORD INDEX; whoever finds a slot taken compares its key with the
//             owner's record in global memory (complete before this launch), so nobody ever waits for a winner's write --
//             winner and loser may sit in one wave.  32 probes, then the record goes to an overflow list that is streamed
//             from global memory in every step (still exact: the sums are additive).  (2) each thread keeps its 2 slots in
//             registers; per candidate, in rank order: masked sums of area and intersection, a wave reduction, one
//             barrier (double-buffered partials), the fp64 comparison, the accepted set updated in registers:
//             <= 128 steps of (2 slots + overflow / 1024) keys per thread.  (3) stuff areas = total[label] - the counts of
//             the keys of that label that meet the accepted set; ids, the rank -> id and label -> id tables, `segments`
//             (rows behind `count` zeroed), `count`, `stats`.
//   write     flat over the image, 4 pixels per thread: lowest accepted rank of the set -> its id, else the label's id or
//             0; 16-B loads of the set words, one 16-B store: (4 ceil(R / 32) + 8 + 4) B per pixel.
// Pasted source, region prepass against reading every candidate's row: only the second is built and measured here (the
// numbers are in DESIGN.md 3.16); the fused source is the one that skips by region.
#pragma clang fp contract(off)
#include "common.h"

namespace d2amd {

constexpr int PAN_MAX_R = 128, PAN_MAX_CLASSES = 256, PAN_BINS = 257;  // bin 256: labels outside [0, num_classes)
constexpr int PAN_TILE_W = 64, PAN_TILE_H = 16, PAN_BLOCK = 256;
constexpr int PAN_STAGE_FLOATS = 8192;  // 32 KB of LDS for the staged masks (and, afterwards, the tile's records)
constexpr int PAN_TABLE = 2048, PAN_GREEDY_BLOCK = 1024, PAN_PROBES = 32;
constexpr int PAN_REC = 6;  // words of a record: set[4], label, count

struct PanHeader {  // the head of the workspace
  int ncand, nrec, pad0, pad1;
  uint32_t acc[4];          // the accepted set
  int order[PAN_MAX_R];     // rank -> detection
  int rank2id[PAN_MAX_R];
  int label2id[PAN_BINS + 3];
  uint32_t total[PAN_BINS + 3];  // pixels per label bin
};

__global__ __launch_bounds__(PAN_MAX_R) void panoptic_rank_kernel(const float* __restrict__ scores, int R, double thresh,
                                                                  PanHeader* __restrict__ hd) {
  __shared__ float s_sc[PAN_MAX_R];
  __shared__ int s_c[PAN_MAX_R];
  const int t = threadIdx.x;
  const float s = t < R ? scores[t] : 0.f;
  const bool cand = t < R && (double)s >= thresh;
  s_sc[t] = s;
  s_c[t] = cand;
  __syncthreads();
  int rank = 0, n = 0;
  for (int j = 0; j < R; j++) {
    if (!s_c[j]) continue;
    n++;
    const float sj = s_sc[j];
    rank += (sj > s || (sj == s && j < t)) ? 1 : 0;
  }
  if (cand) hd->order[rank] = t;
  if (t == 0) {
    hd->ncand = n;
    hd->nrec = 0;
  }
  if (t < 4) hd->acc[t] = 0u;
  for (int i = t; i < PAN_BINS + 3; i += PAN_MAX_R) hd->total[i] = 0u;
}

__device__ __forceinline__ uint32_t pan_prev_lane(uint32_t v) {  // the value of lane - 1 inside a row of 16 lanes
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111 /* row_shr:1 */, 0xf, 0xf, false);
}

template <bool FUSED, typename T>
__global__ __launch_bounds__(PAN_BLOCK) void panoptic_coverage_kernel(
    const uint8_t* __restrict__ masks, const T* __restrict__ probs, const float* __restrict__ boxes,
    const int64_t* __restrict__ sem, int H, int W, int M, float threshold, int num_classes, int nw,
    PanHeader* __restrict__ hd, uint32_t* __restrict__ planes, long plane_stride, uint32_t* __restrict__ recs) {
  __shared__ __attribute__((aligned(16))) float s_stage[PAN_STAGE_FLOATS];
  __shared__ float s_box[PAN_MAX_R][4];
  __shared__ int s_reg[PAN_MAX_R][4];
  __shared__ int s_det[PAN_MAX_R], s_list[PAN_MAX_R], s_meet[PAN_MAX_R];
  __shared__ uint32_t s_hist[PAN_BINS];
  __shared__ int s_n, s_nrec, s_base;
  const int tid = threadIdx.x, lane = tid & 63;
  const int ncand = hd->ncand;
  const int tx0 = blockIdx.x * PAN_TILE_W, ty0 = blockIdx.y * PAN_TILE_H;
  const int y = ty0 + (tid >> 4), x = tx0 + (tid & 15) * 4;
  for (int i = tid; i < PAN_BINS; i += PAN_BLOCK) s_hist[i] = 0u;
  if (tid == 0) s_nrec = 0;
  if (tid < PAN_MAX_R) {
    bool meets = false;
    if (tid < ncand) {
      const int d = hd->order[tid];
      s_det[tid] = d;
      meets = true;
      if (FUSED) {
        // the region that can hold a non-zero sample: paste_region_kernel's rule, operation for operation
        const float x0 = boxes[d * 4 + 0], y0 = boxes[d * 4 + 1], x1 = boxes[d * 4 + 2], y1 = boxes[d * 4 + 3];
        const float mx = ceilf(fabsf(x1 - x0) / (2.f * (float)M)) + 1.f, my = ceilf(fabsf(y1 - y0) / (2.f * (float)M)) + 1.f;
        float fx0 = floorf(fminf(x0, x1)) - 1.f - mx, fy0 = floorf(fminf(y0, y1)) - 1.f - my;
        float fx1 = ceilf(fmaxf(x0, x1)) + 1.f + mx, fy1 = ceilf(fmaxf(y0, y1)) + 1.f + my;
        if (!(fx0 == fx0 && fx1 == fx1 && fy0 == fy0 && fy1 == fy1)) { fx0 = fy0 = 0.f; fx1 = (float)W; fy1 = (float)H; }  // NaN box
        fx0 = fx0 < 0.f ? 0.f : fx0;
        fy0 = fy0 < 0.f ? 0.f : fy0;
        fx1 = fx1 > (float)W ? (float)W : fx1;
        fy1 = fy1 > (float)H ? (float)H : fy1;
        const int rx0 = (int)fx0, ry0 = (int)fy0, rx1 = (int)fx1, ry1 = (int)fy1;
        s_box[tid][0] = x0; s_box[tid][1] = y0; s_box[tid][2] = x1; s_box[tid][3] = y1;
        s_reg[tid][0] = rx0; s_reg[tid][1] = ry0; s_reg[tid][2] = rx1; s_reg[tid][3] = ry1;
        meets = rx0 < rx1 && ry0 < ry1 && rx0 < tx0 + PAN_TILE_W && rx1 > tx0 && ry0 < ty0 + PAN_TILE_H && ry1 > ty0;
      }
    }
    s_meet[tid] = meets ? 1 : 0;
  }
  __syncthreads();
  if (FUSED && tid < PAN_MAX_R) {  // compaction in rank order
    int pos = 0;
    for (int j = 0; j < tid; j++) pos += s_meet[j];
    if (s_meet[tid]) s_list[pos] = tid;
    if (tid == PAN_MAX_R - 1) s_n = pos + s_meet[tid];
  }
  __syncthreads();

  uint32_t set[4][4];  // [pixel][word], every index static
#pragma unroll
  for (int j = 0; j < 4; j++)
#pragma unroll
    for (int k = 0; k < 4; k++) set[j][k] = 0u;

  if (FUSED) {
    const int n = s_n, mm = M * M, per = PAN_STAGE_FLOATS / mm;
    const float sx = (float)M / 2.f, sy = (float)M / 2.f;
    for (int b0 = 0; b0 < n; b0 += per) {
      const int nb = min(per, n - b0);
      if (b0 > 0) __syncthreads();  // the previous batch has been sampled
      for (int i = tid; i < nb * mm; i += PAN_BLOCK) {
        const int q = i / mm, e = i - q * mm;
        s_stage[i] = to_f32(probs[(long)s_det[s_list[b0 + q]] * mm + e]);
      }
      __syncthreads();
      if (y < H) {
        for (int q = 0; q < nb; q++) {
          const int r = s_list[b0 + q];
          const int rx0 = s_reg[r][0], ry0 = s_reg[r][1], rx1 = s_reg[r][2], ry1 = s_reg[r][3];
          if (y < ry0 || y >= ry1 || x + 3 < rx0 || x >= rx1) continue;
          const float* smask = s_stage + q * mm;
          const float x0 = s_box[r][0], y0 = s_box[r][1], x1 = s_box[r][2], y1 = s_box[r][3];
          const float dxw = x1 - x0, dyh = y1 - y0;
          const float gy = ((float)y + 0.5f - y0) / dyh * 2.f - 1.f;
          const float iy = __builtin_fmaf(gy + 1.f, sy, -0.5f);
          const float fly = floorf(iy);
          const bool yfin = fly > -4.0e8f && fly < 4.0e8f;
          const int yn = yfin ? (int)fly : 0;
          const float nn = iy - fly, s_ = 1.f - nn;
          const bool y0ok = yn >= 0 && yn < M, y1ok = yn + 1 >= 0 && yn + 1 < M;
          const int wk = r >> 5;
          const uint32_t bit = 1u << (r & 31);
#pragma unroll
          for (int j = 0; j < 4; j++) {
            const int px = x + j;
            if (px < rx0 || px >= rx1) continue;
            const float gx = ((float)px + 0.5f - x0) / dxw * 2.f - 1.f;
            const float ix = __builtin_fmaf(gx + 1.f, sx, -0.5f);
            const float flx = floorf(ix);
            float val = 0.f;
            if (flx > -4.0e8f && flx < 4.0e8f && yfin) {
              const int xw = (int)flx;
              const float w = ix - flx, e = 1.f - w;
              const float nw_ = s_ * e, ne = s_ * w, sw = nn * e, se = nn * w;
              const bool x0ok = xw >= 0 && xw < M, x1ok = xw + 1 >= 0 && xw + 1 < M;
              const float v00 = (y0ok && x0ok) ? smask[yn * M + xw] : 0.f;
              const float v01 = (y0ok && x1ok) ? smask[yn * M + xw + 1] : 0.f;
              const float v10 = (y1ok && x0ok) ? smask[(yn + 1) * M + xw] : 0.f;
              const float v11 = (y1ok && x1ok) ? smask[(yn + 1) * M + xw + 1] : 0.f;
              val = v00 * nw_;
              val = __builtin_fmaf(v01, ne, val);
              val = __builtin_fmaf(v10, sw, val);
              val = __builtin_fmaf(v11, se, val);
            }
            const uint32_t hit = val >= threshold ? bit : 0u;
#pragma unroll
            for (int k = 0; k < 4; k++) set[j][k] |= (k == wk) ? hit : 0u;
          }
        }
      }
    }
  } else if (y < H && x < W) {
    // The thread's 4 mask bytes of one candidate as the aligned dword(s) that hold them, 8 candidates in flight.  Rows
    // are W bytes apart, so most rows start off a dword boundary: the two dwords are funnel-shifted.  Both hold at least
    // one byte of the thread's own four (the second is only read when the first does not hold all of them), and an
    // aligned dword never crosses a page.  The last thread of a row (x + 3 >= W) reads its bytes one by one.
    const long rowoff = (long)y * W + x, hw = (long)H * W;
    const bool four = x + 3 < W;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int rend = min(32, ncand - 32 * k);
      for (int b0 = 0; b0 < rend; b0 += 8) {
        uint32_t v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
          v[u] = 0u;
          if (b0 + u >= rend) continue;
          const uint8_t* p = masks + (long)s_det[32 * k + b0 + u] * hw + rowoff;
          if (four) {
            const uint32_t off = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 3u);
            const uint32_t* q = reinterpret_cast<const uint32_t*>(p - off);
            const uint32_t lo = q[0], hi = q[off ? 1 : 0];
            v[u] = (uint32_t)((((unsigned long long)hi << 32) | lo) >> (8 * off));
          } else {
#pragma unroll
            for (int j = 0; j < 4; j++)
              if (x + j < W && p[j] != 0) v[u] |= 0xffu << (8 * j);
          }
        }
#pragma unroll
        for (int u = 0; u < 8; u++)
#pragma unroll
          for (int j = 0; j < 4; j++) set[j][k] |= ((v[u] >> (8 * j)) & 0xffu) ? (1u << ((b0 + u) & 31)) : 0u;
      }
    }
  }

  // ---- labels, set planes, histogram
  bool in[4], cov[4];
  uint32_t lab[4];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    in[j] = y < H && x + j < W;
    lab[j] = PAN_MAX_CLASSES;
    if (in[j]) {
      const int64_t l = sem[(long)y * W + x + j];
      if (l >= 0 && l < (int64_t)num_classes) lab[j] = (uint32_t)l;
    }
    cov[j] = in[j] && (set[j][0] | set[j][1] | set[j][2] | set[j][3]) != 0u;
  }
  if (in[0]) {
    const long base = (long)y * W + x;
    const bool vec = in[3] && (base & 3) == 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      if (k >= nw) continue;
      uint32_t* pl = planes + (long)k * plane_stride + base;
      if (vec) {
        *reinterpret_cast<uint4*>(pl) = make_uint4(set[0][k], set[1][k], set[2][k], set[3][k]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++)
          if (in[j]) pl[j] = set[j][k];
      }
    }
    if (in[3] && lab[0] == lab[1] && lab[0] == lab[2] && lab[0] == lab[3]) {
      atomicAdd(&s_hist[lab[0]], 4u);
    } else {
#pragma unroll
      for (int j = 0; j < 4; j++)
        if (in[j]) atomicAdd(&s_hist[lab[j]], 1u);
    }
  }

  // ---- records of the covered pixels.  same[j]: pixel j continues pixel j - 1's key
  bool same[4];
  same[0] = false;
#pragma unroll
  for (int j = 1; j < 4; j++)
    same[j] = cov[j] && cov[j - 1] && lab[j] == lab[j - 1] && set[j][0] == set[j - 1][0] && set[j][1] == set[j - 1][1] &&
              set[j][2] == set[j - 1][2] && set[j][3] == set[j - 1][3];
  const bool uni = cov[0] && same[1] && same[2] && same[3];  // one key for the thread's four pixels
  // a uniform thread continues the uniform thread on its left (same image row: rows are 16 lanes) when the keys agree
  // (every DPP read is made by all 64 lanes, before any of the results is combined)
  const uint32_t pu = pan_prev_lane(uni ? 1u : 0u), p0 = pan_prev_lane(set[0][0]), p1 = pan_prev_lane(set[0][1]),
                 p2 = pan_prev_lane(set[0][2]), p3 = pan_prev_lane(set[0][3]), pl = pan_prev_lane(lab[0]);
  const bool cont = uni & ((lane & 15) != 0) & (pu != 0u) & (p0 == set[0][0]) & (p1 == set[0][1]) & (p2 == set[0][2]) &
                    (p3 == set[0][3]) & (pl == lab[0]);
  const unsigned long long contm = __ballot(cont);
  const unsigned long long rest = lane == 63 ? 0ull : (contm >> (lane + 1));
  const uint32_t run = 1u + (uint32_t)__builtin_ctzll(~rest);  // uniform threads of this key from here on
  uint32_t cnt[4];  // count of the record that STARTS at pixel j, 0 = none
  if (uni) {
    cnt[0] = cont ? 0u : 4u * run;
    cnt[1] = cnt[2] = cnt[3] = 0u;
  } else {
    // run lengths inside the thread, from the right
    uint32_t len[4];
    len[3] = 1u;
#pragma unroll
    for (int j = 2; j >= 0; j--) len[j] = 1u + (same[j + 1] ? len[j + 1] : 0u);
#pragma unroll
    for (int j = 0; j < 4; j++) cnt[j] = (cov[j] && !same[j]) ? len[j] : 0u;
  }
  const int mine = (cnt[0] != 0u) + (cnt[1] != 0u) + (cnt[2] != 0u) + (cnt[3] != 0u);
  int incl = mine;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int v = __shfl_up(incl, d, 64);
    if (lane >= d) incl += v;
  }
  __syncthreads();  // every wave is done with the staged masks: s_stage becomes the tile's record buffer
  int wbase = 0;
  if (lane == 63 && incl > 0) wbase = atomicAdd(&s_nrec, incl);  // one LDS atomic per wave
  wbase = __shfl(wbase, 63, 64);
  uint32_t* s_rec = reinterpret_cast<uint32_t*>(s_stage);
  int slot = wbase + incl - mine;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    if (cnt[j] == 0u) continue;
    uint32_t* r = s_rec + slot * PAN_REC;
    r[0] = set[j][0]; r[1] = set[j][1]; r[2] = set[j][2]; r[3] = set[j][3]; r[4] = lab[j]; r[5] = cnt[j];
    slot++;
  }
  __syncthreads();
  const int nrec = s_nrec;
  if (tid == 0 && nrec > 0) s_base = atomicAdd(&hd->nrec, nrec);  // one global atomic per workgroup
  for (int i = tid; i < PAN_BINS; i += PAN_BLOCK)
    if (s_hist[i] != 0u) atomicAdd(&hd->total[i], s_hist[i]);
  __syncthreads();
  if (nrec > 0) {
    uint32_t* dst = recs + (long)s_base * PAN_REC;
    for (int i = tid; i < nrec * PAN_REC; i += PAN_BLOCK) dst[i] = s_rec[i];
  }
}

__device__ __forceinline__ uint32_t pan_hash(const uint32_t (&k)[5]) {
  uint32_t h = k[0] * 0x9E3779B1u;
  h = (h ^ (h >> 15)) + k[1] * 0x85EBCA6Bu;
  h = (h ^ (h >> 13)) + k[2] * 0xC2B2AE35u;
  h = (h ^ (h >> 16)) + k[3] * 0x27D4EB2Fu;
  h = (h ^ (h >> 15)) + k[4] * 0x165667B1u;
  h ^= h >> 16;
  h *= 0x7FEB352Du;
  h ^= h >> 15;
  return h;
}

// the two sums of one key for candidate bit (wk, bit): its pixels when the key holds the candidate, and those of them
// an accepted thing already owns
__device__ __forceinline__ void pan_step_add(const uint32_t (&s)[4], uint32_t c, int wk, uint32_t bit,
                                             const uint32_t (&acc)[4], uint32_t& area, uint32_t& inter) {
  uint32_t w = 0u;
#pragma unroll
  for (int k = 0; k < 4; k++) w |= (k == wk) ? s[k] : 0u;
  if (w & bit) {
    area += c;
    if (((s[0] & acc[0]) | (s[1] & acc[1]) | (s[2] & acc[2]) | (s[3] & acc[3])) != 0u) inter += c;
  }
}

__global__ __launch_bounds__(PAN_GREEDY_BLOCK) void panoptic_greedy_kernel(
    PanHeader* __restrict__ hd, const uint32_t* __restrict__ recs, int* __restrict__ ovf,
    const int64_t* __restrict__ pred_classes, int R, int num_classes, double overlap_thr, double stuff_thr,
    int64_t* __restrict__ segments, int64_t* __restrict__ count_out, int64_t* __restrict__ stats_out) {
  __shared__ int s_tag[PAN_TABLE];  // 0 = free, else 1 + the record that owns the slot
  __shared__ uint32_t s_cnt[PAN_TABLE];
  __shared__ uint32_t s_part[2][PAN_GREEDY_BLOCK / 64][2];
  __shared__ uint32_t s_owned[PAN_BINS], s_area[PAN_BINS];
  __shared__ int s_keep[PAN_BINS];
  __shared__ int s_novf, s_count;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nrec = hd->nrec, ncand = hd->ncand;
  for (int i = tid; i < PAN_TABLE; i += PAN_GREEDY_BLOCK) { s_tag[i] = 0; s_cnt[i] = 0u; }
  for (int i = tid; i < PAN_BINS; i += PAN_GREEDY_BLOCK) s_owned[i] = 0u;
  if (tid == 0) s_novf = 0;
  __syncthreads();

  // ---- (1) distinct keys.  No thread waits for another: a taken slot names the record whose key it holds
  for (int i = tid; i < nrec; i += PAN_GREEDY_BLOCK) {
    uint32_t key[5];
#pragma unroll
    for (int k = 0; k < 5; k++) key[k] = recs[(long)i * PAN_REC + k];
    const uint32_t c = recs[(long)i * PAN_REC + 5];
    const uint32_t h = pan_hash(key);
    bool done = false;
    for (int p = 0; p < PAN_PROBES && !done; p++) {
      const int slot = (int)((h + (uint32_t)p) & (PAN_TABLE - 1));
      // (a tag changes once, from 0: a taken slot is seen by a plain read, and only a free one costs the atomic)
      int prev = __hip_atomic_load(&s_tag[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (prev == 0) prev = atomicCAS(&s_tag[slot], 0, i + 1);
      bool eq = prev == 0;
      if (!eq) {
        const uint32_t* o = recs + (long)(prev - 1) * PAN_REC;
        eq = o[0] == key[0] && o[1] == key[1] && o[2] == key[2] && o[3] == key[3] && o[4] == key[4];
      }
      if (eq) {
        atomicAdd(&s_cnt[slot], c);
        done = true;
      }
    }
    if (!done) ovf[atomicAdd(&s_novf, 1)] = i;
  }
  __syncthreads();
  const int novf = s_novf;
  uint32_t eset[2][4], ecnt[2], elab[2];  // this thread's two slots
#pragma unroll
  for (int e = 0; e < 2; e++) {
    const int slot = tid + e * PAN_GREEDY_BLOCK;
    const int tag = s_tag[slot];
    ecnt[e] = tag ? s_cnt[slot] : 0u;
    const uint32_t* o = recs + (long)(tag ? tag - 1 : 0) * PAN_REC;
#pragma unroll
    for (int k = 0; k < 4; k++) eset[e][k] = tag ? o[k] : 0u;
    elab[e] = tag ? o[4] : 0u;
  }

  // ---- (2) the greedy pass, in rank order
  uint32_t acc[4] = {0u, 0u, 0u, 0u};
  int next = 0;
  for (int r = 0; r < ncand; r++) {
    const int wk = r >> 5;
    const uint32_t bit = 1u << (r & 31);
    uint32_t area = 0u, inter = 0u;
#pragma unroll
    for (int e = 0; e < 2; e++) pan_step_add(eset[e], ecnt[e], wk, bit, acc, area, inter);
    for (int o = tid; o < novf; o += PAN_GREEDY_BLOCK) {  // keys beyond the table: streamed
      const uint32_t* q = recs + (long)ovf[o] * PAN_REC;
      const uint32_t s[4] = {q[0], q[1], q[2], q[3]};
      pan_step_add(s, q[5], wk, bit, acc, area, inter);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { area += __shfl_xor(area, d); inter += __shfl_xor(inter, d); }
    if (lane == 0) { s_part[r & 1][wave][0] = area; s_part[r & 1][wave][1] = inter; }
    __syncthreads();  // (the other buffer is written next: one barrier per step)
    uint32_t a = 0u, it = 0u;
#pragma unroll
    for (int w = 0; w < PAN_GREEDY_BLOCK / 64; w++) { a += s_part[r & 1][w][0]; it += s_part[r & 1][w][1]; }
    if (a == 0u || (double)it / (double)a > overlap_thr) continue;  // uniform
    next++;
#pragma unroll
    for (int k = 0; k < 4; k++) acc[k] |= (k == wk) ? bit : 0u;
    if (tid == 0) {
      const int d = hd->order[r];
      hd->rank2id[r] = next;
      int64_t* row = segments + (long)(next - 1) * 5;
      row[0] = next; row[1] = 1; row[2] = pred_classes[d]; row[3] = d; row[4] = (int64_t)(a - it);
    }
  }

  // ---- (3) stuff
#pragma unroll
  for (int e = 0; e < 2; e++)
    if (ecnt[e] != 0u && ((eset[e][0] & acc[0]) | (eset[e][1] & acc[1]) | (eset[e][2] & acc[2]) | (eset[e][3] & acc[3])) != 0u)
      atomicAdd(&s_owned[elab[e]], ecnt[e]);
  for (int o = tid; o < novf; o += PAN_GREEDY_BLOCK) {
    const uint32_t* q = recs + (long)ovf[o] * PAN_REC;
    if (((q[0] & acc[0]) | (q[1] & acc[1]) | (q[2] & acc[2]) | (q[3] & acc[3])) != 0u) atomicAdd(&s_owned[q[4]], q[5]);
  }
  __syncthreads();
  if (tid < PAN_BINS) {
    const uint32_t total = hd->total[tid], area = total - s_owned[tid];
    // a label takes part when it occurs in the image (the reference's torch.unique), label 0 never
    s_keep[tid] = (tid >= 1 && tid < num_classes && total != 0u && !((double)area < stuff_thr)) ? 1 : 0;
    s_area[tid] = area;
  }
  __syncthreads();
  if (tid < PAN_BINS) {
    int before = 0;
    for (int j = 0; j < tid; j++) before += s_keep[j];
    const int id = next + before + 1;
    hd->label2id[tid] = s_keep[tid] ? id : 0;
    if (s_keep[tid]) {
      int64_t* row = segments + (long)(id - 1) * 5;
      row[0] = id; row[1] = 0; row[2] = tid; row[3] = -1; row[4] = (int64_t)s_area[tid];
    }
    if (tid == PAN_BINS - 1) s_count = next + before;  // (bin 256 is never kept)
  }
  if (tid < 4) hd->acc[tid] = acc[tid];
  __syncthreads();
  const int count = s_count;
  for (int i = count * 5 + tid; i < (R + num_classes) * 5; i += PAN_GREEDY_BLOCK) segments[i] = 0;
  if (tid == 0) {
    count_out[0] = count;
    stats_out[0] = (int64_t)hd->total[PAN_MAX_CLASSES];
  }
}

__device__ __forceinline__ int pan_pixel_id(const uint32_t (&m)[4], int64_t l, int num_classes, const int* r2i,
                                            const int* l2i) {
  int rank = -1;
#pragma unroll
  for (int k = 3; k >= 0; k--)
    if (m[k] != 0u) rank = 32 * k + __builtin_ctz(m[k]);
  if (rank >= 0) return r2i[rank];
  return (l >= 0 && l < (int64_t)num_classes) ? l2i[(int)l] : 0;
}

__global__ __launch_bounds__(PAN_BLOCK) void panoptic_write_kernel(
    const PanHeader* __restrict__ hd, const uint32_t* __restrict__ planes, long plane_stride,
    const int64_t* __restrict__ sem, long hw, int nw, int num_classes, int32_t* __restrict__ out) {
  __shared__ int s_r2i[PAN_MAX_R], s_l2i[PAN_BINS];
  const int tid = threadIdx.x;
  const int ncand = hd->ncand;
  if (tid < PAN_MAX_R) s_r2i[tid] = tid < ncand ? hd->rank2id[tid] : 0;  // (read only at accepted ranks)
  for (int i = tid; i < PAN_BINS; i += PAN_BLOCK) s_l2i[i] = hd->label2id[i];
  const uint32_t acc[4] = {hd->acc[0], hd->acc[1], hd->acc[2], hd->acc[3]};
  __syncthreads();
  const long i0 = ((long)blockIdx.x * PAN_BLOCK + tid) * 4;
  if (i0 >= hw) return;
  if (i0 + 3 < hw) {
    uint32_t m[4][4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (k < nw) v = *reinterpret_cast<const uint4*>(planes + (long)k * plane_stride + i0);
      m[0][k] = v.x & acc[k]; m[1][k] = v.y & acc[k]; m[2][k] = v.z & acc[k]; m[3][k] = v.w & acc[k];
    }
    int4 o;
    o.x = pan_pixel_id(m[0], sem[i0 + 0], num_classes, s_r2i, s_l2i);
    o.y = pan_pixel_id(m[1], sem[i0 + 1], num_classes, s_r2i, s_l2i);
    o.z = pan_pixel_id(m[2], sem[i0 + 2], num_classes, s_r2i, s_l2i);
    o.w = pan_pixel_id(m[3], sem[i0 + 3], num_classes, s_r2i, s_l2i);
    *reinterpret_cast<int4*>(out + i0) = o;
  } else {
    for (long i = i0; i < hw; i++) {
      uint32_t m[4];
#pragma unroll
      for (int k = 0; k < 4; k++) m[k] = k < nw ? (planes[(long)k * plane_stride + i] & acc[k]) : 0u;
      out[i] = pan_pixel_id(m, sem[i], num_classes, s_r2i, s_l2i);
    }
  }
}

static inline size_t pan_align16(size_t v) { return (v + 15) & ~(size_t)15; }
static inline size_t pan_plane_stride(int H, int W) { return ((size_t)H * W + 3) & ~(size_t)3; }

template <bool FUSED, typename T>
static void launch_coverage(dim3 grid, hipStream_t s, const uint8_t* masks, const void* probs, const float* boxes,
                            const int64_t* sem, int H, int W, int M, float threshold, int num_classes, int nw,
                            PanHeader* hd, uint32_t* planes, long plane_stride, uint32_t* recs) {
  hipLaunchKernelGGL((panoptic_coverage_kernel<FUSED, T>), grid, dim3(PAN_BLOCK), 0, s, masks, (const T*)probs, boxes, sem,
                     H, W, M, threshold, num_classes, nw, hd, planes, plane_stride, recs);
}

}  // namespace d2amd

using namespace d2amd;

extern "C" size_t d2amd_panoptic_workspace_bytes(int H, int W, int R) {
  if (H <= 0 || W <= 0 || R < 0) return 0;
  const size_t hw = (size_t)H * W, nw = ((size_t)R + 31) / 32;
  // header, set planes, one record per pixel at the most, the overflow list of the greedy kernel
  return pan_align16(sizeof(PanHeader)) + nw * pan_plane_stride(H, W) * 4 + pan_align16(hw * PAN_REC * 4) + hw * 4;
}

extern "C" int d2amd_panoptic_combine(const float* scores, const int64_t* pred_classes, const int64_t* semantic,
                                      const uint8_t* pred_masks, const void* mask_probs, const float* boxes, int R,
                                      int H, int W, int M, int mask_dtype, float mask_threshold,
                                      double overlap_threshold, double stuff_area_thresh, double instances_score_thresh,
                                      int num_classes, int32_t* panoptic_seg, int64_t* segments, int64_t* count,
                                      int64_t* stats, void* workspace, size_t workspace_bytes, void* stream) {
  D2_CHECK_ARG(R >= 0 && H > 0 && W > 0 && num_classes > 0, "panoptic_combine: bad shape");
  D2_CHECK_ARG((long)H * W < (1l << 31), "panoptic_combine: H W >= 2^31");
  const bool fused = mask_probs != nullptr;
  if (R > PAN_MAX_R || num_classes > PAN_MAX_CLASSES) {
    set_error("panoptic_combine: R = %d, num_classes = %d (up to %d detections and %d classes are implemented)", R,
              num_classes, PAN_MAX_R, PAN_MAX_CLASSES);
    return D2AMD_EUNSUPPORTED;
  }
  if (R > 0) {
    D2_CHECK_ARG((pred_masks != nullptr) != fused, "panoptic_combine: exactly one of pred_masks / mask_probs");
    D2_CHECK_ARG(scores && pred_classes, "panoptic_combine: null pointer");
  }
  if (fused && R > 0) {
    D2_CHECK_ARG(boxes != nullptr && M > 0, "panoptic_combine: mask_probs need boxes and M > 0");
    D2_CHECK_ARG(mask_threshold >= 0.f, "panoptic_combine: mask_threshold < 0 (the soft uint8 paste) has no coverage");
    if ((size_t)M * M * 4 > (size_t)PAN_STAGE_FLOATS * 4) {
      set_error("panoptic_combine: a %d x %d mask exceeds the %d-byte LDS staging buffer", M, M, PAN_STAGE_FLOATS * 4);
      return D2AMD_EUNSUPPORTED;
    }
    if (mask_dtype != D2AMD_F32 && mask_dtype != D2AMD_F16 && mask_dtype != D2AMD_BF16) {
      set_error("unsupported dtype %d", mask_dtype);
      return D2AMD_EUNSUPPORTED;
    }
  }
  D2_CHECK_ARG(semantic && panoptic_seg && segments && count && stats && workspace, "panoptic_combine: null pointer");
  D2_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 15u) == 0 && (reinterpret_cast<uintptr_t>(panoptic_seg) & 15u) == 0,
               "panoptic_combine: workspace and panoptic_seg must be 16-byte aligned");
  if (workspace_bytes < d2amd_panoptic_workspace_bytes(H, W, R)) {
    set_error("panoptic_combine: workspace of %zu bytes, %zu needed", workspace_bytes, d2amd_panoptic_workspace_bytes(H, W, R));
    return D2AMD_EWORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  const long hw = (long)H * W, plane_stride = (long)pan_plane_stride(H, W);
  const int nw = (R + 31) / 32;
  uint8_t* ws = (uint8_t*)workspace;
  PanHeader* hd = (PanHeader*)ws;
  uint32_t* planes = (uint32_t*)(ws + pan_align16(sizeof(PanHeader)));
  uint32_t* recs = planes + (size_t)nw * plane_stride;
  int* ovf = (int*)((uint8_t*)recs + pan_align16((size_t)hw * PAN_REC * 4));

  hipLaunchKernelGGL(panoptic_rank_kernel, dim3(1), dim3(PAN_MAX_R), 0, s, scores, R, instances_score_thresh, hd);
  D2_LAUNCH_OK();
  const dim3 grid(cdiv(W, PAN_TILE_W), cdiv(H, PAN_TILE_H));
  bool timed = timing_begin("panoptic_coverage", s);
  if (fused && R > 0) {
    const int rc = D2_DISPATCH_DTYPE(mask_dtype, [&]() -> int {
      launch_coverage<true, scalar_t>(grid, s, nullptr, mask_probs, boxes, semantic, H, W, M, mask_threshold, num_classes,
                                      nw, hd, planes, plane_stride, recs);
      return D2AMD_OK;
    });
    if (rc != D2AMD_OK) return rc;
  } else {
    launch_coverage<false, float>(grid, s, pred_masks, nullptr, nullptr, semantic, H, W, 1, 0.f, num_classes, nw, hd,
                                  planes, plane_stride, recs);
  }
  if (timed) timing_end("panoptic_coverage", s);
  D2_LAUNCH_OK();
  timed = timing_begin("panoptic_greedy", s);
  hipLaunchKernelGGL(panoptic_greedy_kernel, dim3(1), dim3(PAN_GREEDY_BLOCK), 0, s, hd, recs, ovf, pred_classes, R,
                     num_classes, overlap_threshold, stuff_area_thresh, segments, count, stats);
  if (timed) timing_end("panoptic_greedy", s);
  D2_LAUNCH_OK();
  timed = timing_begin("panoptic_write", s);
  hipLaunchKernelGGL(panoptic_write_kernel, dim3(cdiv(cdiv(hw, 4), PAN_BLOCK)), dim3(PAN_BLOCK), 0, s, hd, planes,
                     plane_stride, semantic, hw, nw, num_classes, panoptic_seg);
  if (timed) timing_end("panoptic_write", s);
  D2_LAUNCH_OK();
  return D2AMD_OK;
}
