// Keypoint R-CNN head glue either side of the keypoint head's convolutions.
//   replaces  detectron2/structures/keypoints.py:104-161 (_keypoints_to_heatmap: ~25 elementwise launches),
//             detectron2/modeling/roi_heads/keypoint_head.py:40-96 (keypoint_rcnn_loss: nonzero -- a host sync --, a
//             gathered copy pred[valid] of up to N*K rows of S*S logits, cross_entropy, and in the backward an index_put
//             into a zero-filled tensor) and
//             detectron2/structures/keypoints.py:165-235 (heatmaps_to_keypoints: a Python loop over the ROIs with two host
//             reads, a bicubic F.interpolate to the ROI's pixel size, ~10 small ops and a synchronising assert per ROI).
// Here:
//   * targets: one __device__ function (kp_target), fp32 in the reference's op order (no contraction: this file is
//     compiled with -ffp-contract=off), shared by the stand-alone target kernel and the loss.
//   * loss forward: ONE WAVE PER ROW (n, k), four rows per workgroup.  The row (S*S logits, <= 4,096) is loaded once with
//     16-byte loads and stays in registers (<= 64 fp32 per lane); max and sum(exp) are cross-lane butterflies: one HBM
//     read, no LDS.  Invalid rows read nothing.  lse / target / row loss go to the workspace; a second one-workgroup
//     launch adds the row losses in a fixed order (deterministic, no float atomics) and counts the valid rows.
//   * loss backward: same mapping; (exp(x - lse) - onehot) * g / normalizer for valid rows, zeros (written without
//     reading the logits) for the others; the whole (N, K, S, S) gradient is written exactly once.  The number of valid
//     rows comes from the workspace: no host read anywhere.
//   * decode: ONE WORKGROUP (1,024 threads) PER (ROI, keypoint).  The S x S map is staged in LDS as fp32 once; the bicubic
//     resize to the ROI's H' x W' pixels is done SEPARABLY over strips of 128 output columns: a horizontal pass writes
//     T[S][strip] to LDS (each lane owns a column and computes its four x-weights once); in the vertical pass a lane owns
//     two columns, the 16 waves share the output rows (of a narrow ROI too), and the y-taps -- the same for every lane --
//     are computed once per row and fetched with v_readlane: 4 LDS reads + 4 FMAs per output pixel and a running
//     (max, row) in registers.  ~4 + 4 S / H' MACs per output pixel instead of 16; the upsampled map is never written
//     anywhere.  Every tap index is computed and clamped per output coordinate, so downsampling (ROIs smaller than S px)
//     takes the same code.
//     MFMA does not fit: the interpolation operator has 4 nonzeros per row of S (a dense matmul does S / 4 = 14 x the work
//     at S = 56, and it is banded only when upsampling), and the argmax needs the full fp32 result.
// Roofline: the loss is HBM-bound: forward reads rows_valid * S*S * s bytes, backward reads the same and writes
// N*K*S*S * s bytes (N = 256, K = 17, fp32: 54.6 MB each).  The decode is LDS / VALU-bound (10.7 MB of maps at R = 100).
#include "common.h"

namespace d2amd {

constexpr int KP_MAX_S = 64;             // side of the heatmap: 2 <= S <= 64
constexpr int KP_ROW_REGS = 64;          // fp32 values of a row one lane holds: 64 * 64 / 64
constexpr int KP_STRIP = 128;            // output columns per strip of the decode (two per lane of a wave)
constexpr int KP_DEC_THREADS = 1024;     // decode workgroup: 16 waves share the output rows of one (ROI, keypoint)
constexpr int KP_MAX_EXTENT = 16384;     // H', W' are clamped to this many pixels (pos stays far below 2^31)

struct KpHeader { int64_t valid_rows; int64_t pad; };  // head of the loss workspace; then lse[rows], target[rows], loss[rows]

// ---- targets (keypoints.py:104-161) ----------------------------------------------------------------------------
// -> y * S + x of the keypoint's cell, or -1 when the keypoint does not count (outside the box, not labelled, or a box
// of zero / NaN extent: the reference casts inf / nan to an integer there, which is undefined).
// `S / (x2 - x1)` with a Python int on the left is reciprocal(x2 - x1) * S in torch: two roundings, kept.
__device__ __forceinline__ int kp_target(const float* __restrict__ kp, const float* __restrict__ roi, int S) {
  const float x1 = roi[0], y1 = roi[1], x2 = roi[2], y2 = roi[3];
  const float fs = (float)S;
  const float sx = (1.f / (x2 - x1)) * fs;
  const float sy = (1.f / (y2 - y1)) * fs;
  const float x = kp[0], y = kp[1], vis = kp[2];
  float fx = floorf((x - x1) * sx);
  float fy = floorf((y - y1) * sy);
  if (x == x2) fx = fs - 1.f;
  if (y == y2) fy = fs - 1.f;
  const bool ok = fx >= 0.f && fy >= 0.f && fx < fs && fy < fs && vis > 0.f && fabsf(sx) < INFINITY &&
                  fabsf(sy) < INFINITY;
  return ok ? (int)fy * S + (int)fx : -1;
}

__global__ __launch_bounds__(256) void d2amd_kp_targets_kernel(const float* __restrict__ kps,
                                                               const float* __restrict__ rois, long rows, int K, int S,
                                                               int64_t* __restrict__ heatmaps,
                                                               int64_t* __restrict__ valid) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows) return;
  const int t = kp_target(kps + i * 3, rois + (i / K) * 4, S);
  heatmaps[i] = t < 0 ? 0 : t;  // lin_ind * valid
  valid[i] = t < 0 ? 0 : 1;
}

// ---- 16-byte vectors of T <-> fp32 ------------------------------------------------------------------------------
template <typename T> struct kp_vec { static constexpr int N = 16 / (int)sizeof(T); };

__device__ __forceinline__ void kp_load16(const float* p, float (&o)[4]) {
  const float4 v = *reinterpret_cast<const float4*>(p);
  o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
}
template <typename T> __device__ __forceinline__ void kp_load16(const T* p, float (&o)[8]) {
  const uint4 v = *reinterpret_cast<const uint4*>(p);
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int q = 0; q < 4; q++) {
    o[2 * q] = to_f32(T{(uint16_t)(w[q] & 0xffffu)});
    o[2 * q + 1] = to_f32(T{(uint16_t)(w[q] >> 16)});
  }
}
__device__ __forceinline__ void kp_store16(float* p, const float (&i)[4]) {
  *reinterpret_cast<float4*>(p) = make_float4(i[0], i[1], i[2], i[3]);
}
template <typename T> __device__ __forceinline__ void kp_store16(T* p, const float (&i)[8]) {
  uint32_t w[4];
#pragma unroll
  for (int q = 0; q < 4; q++)
    w[q] = (uint32_t)from_f32<T>(i[2 * q]).v | ((uint32_t)from_f32<T>(i[2 * q + 1]).v << 16);
  *reinterpret_cast<uint4*>(p) = uint4{w[0], w[1], w[2], w[3]};
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float wave_sum(float v) {  // butterfly: every lane ends with the same bits
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// exp(d), d <= 0, on the hardware's exp2 (v_exp_f32, 1 ulp): the rounding of d * log2(e) adds |d| e^d 2^-24 <= 2.2e-8 of
// the row's largest term -- the softmax is a unit-scale quantity held to 1e-6.  Measured: the library expf was 4-5 us of
// the forward at 256 x 17 x 56 x 56.
__device__ __forceinline__ float kp_exp(float d) { return __expf(d); }

// ---- loss forward (keypoint_head.py:40-96) ------------------------------------------------------------------
// VEC: rows are whole 16-byte vectors (S*S*sizeof(T) % 16 == 0, aligned base); otherwise element loads.
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void d2amd_kp_loss_rows_kernel(const T* __restrict__ logits,
                                                                 const float* __restrict__ kps,
                                                                 const float* __restrict__ rois, int rows, int K, int S,
                                                                 float* __restrict__ lse_out, int* __restrict__ tgt_out,
                                                                 float* __restrict__ loss_rows) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;  // (whole waves; no barrier below)
  const int tgt = kp_target(kps + (long)row * 3, rois + (long)(row / K) * 4, S);
  if (tgt < 0) {
    if (lane == 0) { lse_out[row] = 0.f; tgt_out[row] = -1; loss_rows[row] = 0.f; }
    return;
  }
  const int HW = S * S;
  const T* x = logits + (long)row * HW;
  constexpr int EPV = kp_vec<T>::N, NV = KP_ROW_REGS / EPV;
  float r[KP_ROW_REGS];
  if (VEC) {
    const int nvec = HW / EPV;
#pragma unroll
    for (int v = 0; v < NV; v++) {
      float e[EPV];
      const int vi = v * 64 + lane;
      if (vi < nvec) {
        kp_load16(x + vi * EPV, e);
      } else {
#pragma unroll
        for (int q = 0; q < EPV; q++) e[q] = -INFINITY;
      }
#pragma unroll
      for (int q = 0; q < EPV; q++) r[v * EPV + q] = e[q];
    }
  } else {
#pragma unroll
    for (int j = 0; j < KP_ROW_REGS; j++) {
      const int i = j * 64 + lane;
      r[j] = i < HW ? to_f32(x[i]) : -INFINITY;
    }
  }
  // slot j holds elements of [j0 * 64, ..): slots wholly behind the row are skipped (the same for every lane)
  const int live = VEC ? (HW / EPV + 63) / 64 * EPV : (HW + 63) / 64;
  float m = -INFINITY;
#pragma unroll
  for (int j = 0; j < KP_ROW_REGS; j++) m = fmaxf(m, r[j]);
  m = wave_max(m);
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < KP_ROW_REGS; j++)
    if (j < live) s += kp_exp(r[j] - m);  // (padding: exp(-inf) = 0)
  s = wave_sum(s);
  if (lane == 0) {
    const float lse = m + logf(s);
    lse_out[row] = lse;
    tgt_out[row] = tgt;
    loss_rows[row] = lse - to_f32(x[tgt]);
  }
}

__global__ __launch_bounds__(256) void d2amd_kp_loss_final_kernel(const float* __restrict__ loss_rows,
                                                                  const int* __restrict__ tgt, int rows,
                                                                  float normalizer, KpHeader* __restrict__ head,
                                                                  float* __restrict__ loss_out,
                                                                  int64_t* __restrict__ stats_out) {
  const int tid = threadIdx.x;
  double loss = 0.;
  long cnt = 0;
  for (int i = tid; i < rows; i += 256) {
    loss += (double)loss_rows[i];
    cnt += tgt[i] >= 0;
  }
  __shared__ double sl[256];
  __shared__ long sc[256];
  sl[tid] = loss; sc[tid] = cnt;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {  // fixed tree: deterministic
    if (tid < s) { sl[tid] += sl[tid + s]; sc[tid] += sc[tid + s]; }
    __syncthreads();
  }
  if (tid == 0) {
    const long n = sc[0];
    const double norm = normalizer > 0.f ? (double)normalizer : (double)n;
    *loss_out = n > 0 ? (float)(sl[0] / norm) : 0.f;
    stats_out[0] = n;
    head->valid_rows = n;
    head->pad = 0;
  }
}

// ---- loss backward ----------------------------------------------------------------------------------------------
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void d2amd_kp_loss_backward_kernel(const T* __restrict__ logits,
                                                                     const KpHeader* __restrict__ head,
                                                                     const float* __restrict__ lse_in,
                                                                     const int* __restrict__ tgt_in,
                                                                     const float* __restrict__ grad_loss, int rows, int S,
                                                                     float normalizer, T* __restrict__ grad) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int HW = S * S;
  const int tgt = tgt_in[row];
  const T* x = logits + (long)row * HW;
  T* g = grad + (long)row * HW;
  constexpr int EPV = kp_vec<T>::N;
  if (tgt < 0) {  // zeros, the logits are not read
    if (VEC) {
      float z[EPV];
#pragma unroll
      for (int q = 0; q < EPV; q++) z[q] = 0.f;
      for (int vi = lane; vi < HW / EPV; vi += 64) kp_store16(g + vi * EPV, z);
    } else {
      for (int i = lane; i < HW; i += 64) g[i] = from_f32<T>(0.f);
    }
    return;
  }
  const float norm = normalizer > 0.f ? normalizer : (float)head->valid_rows;  // (valid_rows >= 1: this row is valid)
  const float scale = *grad_loss / norm;
  const float lse = lse_in[row];
  if (VEC) {
    for (int vi = lane; vi < HW / EPV; vi += 64) {
      float e[EPV];
      kp_load16(x + vi * EPV, e);
#pragma unroll
      for (int q = 0; q < EPV; q++) e[q] = (kp_exp(e[q] - lse) - (vi * EPV + q == tgt ? 1.f : 0.f)) * scale;
      kp_store16(g + vi * EPV, e);
    }
  } else {
    for (int i = lane; i < HW; i += 64)
      g[i] = from_f32<T>((kp_exp(to_f32(x[i]) - lse) - (i == tgt ? 1.f : 0.f)) * scale);
  }
}

// ---- decode (keypoints.py:165-235) --------------------------------------------------------------------------------
// torch's bicubic rule for align_corners=False: source = scale * (dst + 0.5) - 0.5 (not clamped), taps floor(source) - 1 ..
// + 2 clamped to [0, S - 1], cubic-convolution weights (Keys) with A = -0.75.
__device__ __forceinline__ void kp_cubic_taps(float scale, int dst, int S, float (&w)[4], int (&idx)[4]) {
  const float src = scale * ((float)dst + 0.5f) - 0.5f;
  const float fl = floorf(src);
  const float t = src - fl;
  const int i0 = (int)fl - 1;
  constexpr float A = -0.75f;
  const float u = 1.f - t;
  const float t1 = t + 1.f, u1 = u + 1.f;
  w[0] = ((A * t1 - 5.f * A) * t1 + 8.f * A) * t1 - 4.f * A;
  w[1] = ((A + 2.f) * t - (A + 3.f)) * t * t + 1.f;
  w[2] = ((A + 2.f) * u - (A + 3.f)) * u * u + 1.f;
  w[3] = ((A * u1 - 5.f * A) * u1 + 8.f * A) * u1 - 4.f * A;
#pragma unroll
  for (int j = 0; j < 4; j++) idx[j] = min(max(i0 + j, 0), S - 1);
}

// the larger value wins; among exactly equal values the lower linear index
__device__ __forceinline__ void kp_best(float& m, int& p, float v, int q, bool on = true) {
  const bool take = on & ((v > m) | ((v == m) & (q < p)));  // (selects, no branches: the loop below unrolls)
  m = take ? v : m;
  p = take ? q : p;
}

__device__ __forceinline__ float kp_lane_f(float v, int lane) {  // lane: the same for the whole wave
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

template <typename T, bool VEC>
__global__ __launch_bounds__(KP_DEC_THREADS) void d2amd_kp_decode_kernel(const T* __restrict__ maps,
                                                                         const float* __restrict__ rois, int K, int S,
                                                                         float* __restrict__ out,
                                                                         int* __restrict__ pos_out) {
  constexpr int NT = KP_DEC_THREADS, NW = NT / 64;
  __shared__ float smap[KP_MAX_S * KP_MAX_S];   // the S x S map, fp32
  __shared__ float sT[KP_MAX_S * KP_STRIP];     // rows of the map resized horizontally: [S][strip]
  __shared__ float sredv[NW];
  __shared__ int sredp[NW];
  __shared__ float sreds[NW];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long rk = blockIdx.x;
  const long roi = rk / K;
  const int HW = S * S;
  const T* src = maps + rk * HW;
  if (VEC) {
    for (int v = tid; v < HW / 4; v += NT) {
      float e[4];
      unpack4(*reinterpret_cast<const vec4<T>*>(src + v * 4), e);
#pragma unroll
      for (int q = 0; q < 4; q++) smap[v * 4 + q] = e[q];
    }
  } else {
    for (int i = tid; i < HW; i += NT) smap[i] = to_f32(src[i]);
  }
  const float x1 = rois[roi * 4], y1 = rois[roi * 4 + 1], x2 = rois[roi * 4 + 2], y2 = rois[roi * 4 + 3];
  const float w = fmaxf(x2 - x1, 1.f), h = fmaxf(y2 - y1, 1.f);
  const int Wp = (int)fminf(ceilf(w), (float)KP_MAX_EXTENT), Hp = (int)fminf(ceilf(h), (float)KP_MAX_EXTENT);
  const float sx = (float)S / (float)Wp, sy = (float)S / (float)Hp;
  // output rows wave, wave + NW, .. are this wave's, in every strip
  const int cnt = Hp > wave ? (Hp - wave + NW - 1) / NW : 0;

  float best = -INFINITY;
  int bpos = 0;
  for (int x0 = 0; x0 < Wp; x0 += KP_STRIP) {
    const int sw = min(KP_STRIP, Wp - x0);
    __syncthreads();  // the map is staged / the previous strip has been read
    {                 // horizontal pass: a lane owns column c of the strip; the NT / strip groups of lanes share the rows
      const int c = tid & (KP_STRIP - 1);
      if (c < sw) {
        float wx[4];
        int ix[4];
        kp_cubic_taps(sx, x0 + c, S, wx, ix);
        for (int r = tid / KP_STRIP; r < S; r += NT / KP_STRIP) {
          const float* m = smap + r * S;
          float a = wx[0] * m[ix[0]];
          a = fmaf(wx[1], m[ix[1]], a);
          a = fmaf(wx[2], m[ix[2]], a);
          a = fmaf(wx[3], m[ix[3]], a);
          sT[r * KP_STRIP + c] = a;
        }
      }
    }
    __syncthreads();
    // vertical pass: a lane owns columns `lane` and `lane + 64` of the strip, the waves share the output rows (whatever the
    // strip's width: a narrow ROI still uses every wave).  The y-taps are the same for all lanes: lane l computes those of
    // the wave's l-th row of a block of 64 rows, the loop picks row j's with v_readlane -- weights and row offsets sit in
    // scalar registers, a pixel costs 4 LDS reads + 4 FMAs.
    // Within a strip a lane meets its columns' rows in increasing y: "strictly greater" keeps the lowest row, and only the
    // row (a scalar) is recorded -- a compare and two selects per pixel; the general tie rule runs once per strip.
    const float* t = sT + lane;
    float ba = -INFINITY, bb = -INFINITY;
    int ya = 0, yb = 0;
    for (int mb = 0; mb < cnt; mb += 64) {
      float wy[4];
      int iy[4];
      kp_cubic_taps(sy, wave + NW * (mb + lane), S, wy, iy);  // (rows behind Hp: computed, never picked)
      const int o01 = (iy[0] * KP_STRIP) | ((iy[1] * KP_STRIP) << 16);  // offsets into sT: <= 63 * 128
      const int o23 = (iy[2] * KP_STRIP) | ((iy[3] * KP_STRIP) << 16);
      const int n = min(64, cnt - mb);
      for (int j0 = 0; j0 < n; j0 += 4) {  // four rows in flight (j <= 63; rows behind n are computed and dropped)
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const int j = j0 + q;
          const float w0 = kp_lane_f(wy[0], j), w1 = kp_lane_f(wy[1], j), w2 = kp_lane_f(wy[2], j), w3 = kp_lane_f(wy[3], j);
          const int p01 = __builtin_amdgcn_readlane(o01, j), p23 = __builtin_amdgcn_readlane(o23, j);
          const float* r0 = t + (p01 & 0xffff);
          const float* r1 = t + (p01 >> 16);
          const float* r2 = t + (p23 & 0xffff);
          const float* r3 = t + (p23 >> 16);
          float a = w0 * r0[0], b = w0 * r0[64];
          a = fmaf(w1, r1[0], a); b = fmaf(w1, r1[64], b);
          a = fmaf(w2, r2[0], a); b = fmaf(w2, r2[64], b);
          a = fmaf(w3, r3[0], a); b = fmaf(w3, r3[64], b);
          const int y = wave + NW * (mb + j);
          const bool ta = (j < n) & (a > ba), tb = (j < n) & (b > bb);
          ba = ta ? a : ba; ya = ta ? y : ya;
          bb = tb ? b : bb; yb = tb ? y : yb;
        }
      }
    }
    kp_best(best, bpos, ba, ya * Wp + x0 + lane, lane < sw);
    kp_best(best, bpos, bb, yb * Wp + x0 + lane + 64, lane + 64 < sw);
  }
  // (max, lowest position) of the workgroup
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int op = __shfl_xor(bpos, o, 64);
    kp_best(best, bpos, ov, op);
  }
  if (lane == 0) { sredv[wave] = best; sredp[wave] = bpos; }
  __syncthreads();
  float M = sredv[0];
  int P = sredp[0];
#pragma unroll
  for (int q = 1; q < NW; q++) kp_best(M, P, sredv[q], sredp[q]);
  // the score's normaliser runs over the POOL-resolution map with the upsampled maximum (keypoints.py:208-214)
  float s = 0.f;
  for (int i = tid; i < HW; i += NT) s += expf(smap[i] - M);
  s = wave_sum(s);
  if (lane == 0) sreds[wave] = s;
  __syncthreads();
  if (tid == 0) {
    float sum = 0.f;
#pragma unroll
    for (int q = 0; q < NW; q++) sum += sreds[q];  // fixed order
    const int yi = P / Wp, xi = P - yi * Wp;
    float* o = out + rk * 4;
    o[0] = ((float)xi + 0.5f) * (w / (float)Wp) + x1;
    o[1] = ((float)yi + 0.5f) * (h / (float)Hp) + y1;
    o[2] = M;
    o[3] = 1.f / sum;
    if (pos_out) pos_out[rk] = P;
  }
}

}  // namespace d2amd

using namespace d2amd;

#define KP_CHECK_S(op, S) D2_CHECK_ARG((S) >= 2 && (S) <= KP_MAX_S, op ": heatmap side %d outside [2, %d]", (S), KP_MAX_S)

static inline bool kp_rows_vectorise(const void* a, const void* b, int S, int dtype) {
  return ((size_t)S * S * dtype_size(dtype)) % 16 == 0 && ((uintptr_t)a & 15) == 0 && ((uintptr_t)b & 15) == 0;
}

extern "C" int d2amd_keypoints_to_heatmap(const float* keypoints, const float* rois, int N, int K, int S,
                                          int64_t* heatmaps, int64_t* valid, void* stream) {
  D2_CHECK_ARG(N >= 0 && K > 0, "keypoints_to_heatmap: bad shape");
  KP_CHECK_S("keypoints_to_heatmap", S);
  if (N == 0) return D2AMD_OK;
  D2_CHECK_ARG(keypoints && rois && heatmaps && valid, "keypoints_to_heatmap: null pointer");
  const long rows = (long)N * K, nblk = (rows + 255) / 256;
  D2_CHECK_ARG(nblk < (1l << 31), "keypoints_to_heatmap: too many rows");
  hipLaunchKernelGGL(d2amd_kp_targets_kernel, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, keypoints, rois,
                     rows, K, S, heatmaps, valid);
  D2_LAUNCH_OK();
  return D2AMD_OK;
}

extern "C" size_t d2amd_keypoint_rcnn_loss_workspace_bytes(int rows) {
  return sizeof(KpHeader) + (size_t)(rows > 0 ? rows : 1) * 12;
}

extern "C" int d2amd_keypoint_rcnn_loss_forward(const void* logits, const float* keypoints, const float* rois, int N,
                                                int K, int S, int dtype, float normalizer, float* loss_out,
                                                int64_t* stats_out, void* workspace, size_t workspace_bytes,
                                                void* stream) {
  D2_CHECK_ARG(N >= 0 && K > 0, "keypoint_rcnn_loss_forward: bad shape");
  KP_CHECK_S("keypoint_rcnn_loss_forward", S);
  const long rows_l = (long)N * K;
  D2_CHECK_ARG(rows_l < (1l << 29), "keypoint_rcnn_loss_forward: too many rows");
  const int rows = (int)rows_l;
  if (N == 0) return D2AMD_OK;
  D2_CHECK_ARG(workspace && workspace_bytes >= d2amd_keypoint_rcnn_loss_workspace_bytes(rows),
               "keypoint_rcnn_loss_forward: workspace too small (%zu bytes, %zu needed)", workspace_bytes,
               d2amd_keypoint_rcnn_loss_workspace_bytes(rows));
  D2_CHECK_ARG(logits && keypoints && rois && loss_out && stats_out, "keypoint_rcnn_loss_forward: null pointer");
  D2_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "keypoint_rcnn_loss_forward: workspace not 8-byte aligned");
  KpHeader* head = (KpHeader*)workspace;
  float* lse = (float*)(head + 1);
  int* tgt = (int*)(lse + rows);
  float* loss_rows = (float*)(tgt + rows);
  hipStream_t s = (hipStream_t)stream;
  const bool vec = kp_rows_vectorise(logits, logits, S, dtype);
  return D2_DISPATCH_DTYPE(dtype, [&]() -> int {
    if (vec)
      hipLaunchKernelGGL((d2amd_kp_loss_rows_kernel<scalar_t, true>), dim3(cdiv(rows, 4)), dim3(256), 0, s,
                         (const scalar_t*)logits, keypoints, rois, rows, K, S, lse, tgt, loss_rows);
    else
      hipLaunchKernelGGL((d2amd_kp_loss_rows_kernel<scalar_t, false>), dim3(cdiv(rows, 4)), dim3(256), 0, s,
                         (const scalar_t*)logits, keypoints, rois, rows, K, S, lse, tgt, loss_rows);
    D2_LAUNCH_OK();
    hipLaunchKernelGGL(d2amd_kp_loss_final_kernel, dim3(1), dim3(256), 0, s, loss_rows, tgt, rows, normalizer, head,
                       loss_out, stats_out);
    D2_LAUNCH_OK();
    return D2AMD_OK;
  });
}

extern "C" int d2amd_keypoint_rcnn_loss_backward(const void* logits, const void* workspace, const float* grad_loss,
                                                 int N, int K, int S, int dtype, float normalizer, void* grad_logits,
                                                 void* stream) {
  D2_CHECK_ARG(N >= 0 && K > 0, "keypoint_rcnn_loss_backward: bad shape");
  KP_CHECK_S("keypoint_rcnn_loss_backward", S);
  const long rows_l = (long)N * K;
  D2_CHECK_ARG(rows_l < (1l << 29), "keypoint_rcnn_loss_backward: too many rows");
  if (N == 0) return D2AMD_OK;
  D2_CHECK_ARG(logits && workspace && grad_loss && grad_logits, "keypoint_rcnn_loss_backward: null pointer");
  const int rows = (int)rows_l;
  const KpHeader* head = (const KpHeader*)workspace;
  const float* lse = (const float*)(head + 1);
  const int* tgt = (const int*)(lse + rows);
  hipStream_t s = (hipStream_t)stream;
  const bool vec = kp_rows_vectorise(logits, grad_logits, S, dtype);
  return D2_DISPATCH_DTYPE(dtype, [&]() -> int {
    if (vec)
      hipLaunchKernelGGL((d2amd_kp_loss_backward_kernel<scalar_t, true>), dim3(cdiv(rows, 4)), dim3(256), 0, s,
                         (const scalar_t*)logits, head, lse, tgt, grad_loss, rows, S, normalizer, (scalar_t*)grad_logits);
    else
      hipLaunchKernelGGL((d2amd_kp_loss_backward_kernel<scalar_t, false>), dim3(cdiv(rows, 4)), dim3(256), 0, s,
                         (const scalar_t*)logits, head, lse, tgt, grad_loss, rows, S, normalizer, (scalar_t*)grad_logits);
    D2_LAUNCH_OK();
    return D2AMD_OK;
  });
}

extern "C" int d2amd_heatmaps_to_keypoints(const void* maps, const float* rois, int R, int K, int S, int dtype,
                                           float* out, int32_t* pos, void* stream) {
  D2_CHECK_ARG(R >= 0 && K > 0, "heatmaps_to_keypoints: bad shape");
  KP_CHECK_S("heatmaps_to_keypoints", S);
  if (R == 0) return D2AMD_OK;
  D2_CHECK_ARG(maps && rois && out, "heatmaps_to_keypoints: null pointer");
  const long nblk = (long)R * K;
  D2_CHECK_ARG(nblk < (1l << 31), "heatmaps_to_keypoints: too many maps");
  hipStream_t s = (hipStream_t)stream;
  // 4-element vectors of the map: 16 B (fp32) or 8 B (16-bit) loads
  const bool vec = (S * S) % 4 == 0 && ((uintptr_t)maps & (4 * dtype_size(dtype) - 1)) == 0;
  return D2_DISPATCH_DTYPE(dtype, [&]() -> int {
    if (vec)
      hipLaunchKernelGGL((d2amd_kp_decode_kernel<scalar_t, true>), dim3((unsigned)nblk), dim3(KP_DEC_THREADS), 0, s,
                         (const scalar_t*)maps, rois, K, S, out, pos);
    else
      hipLaunchKernelGGL((d2amd_kp_decode_kernel<scalar_t, false>), dim3((unsigned)nblk), dim3(KP_DEC_THREADS), 0, s,
                         (const scalar_t*)maps, rois, K, S, out, pos);
    D2_LAUNCH_OK();
    return D2AMD_OK;
  });
}
