// Semantic-segmentation head glue: the training loss and the label decode of SemSegFPNHead / SemanticSegmentor.
//   replaces  detectron2/modeling/meta_arch/semantic_seg.py:255-267 (SemSegFPNHead.losses: a cast of the stride-s logits
//             to fp32, F.interpolate x s (bilinear, align_corners=False) -- an [N, C, s h, s w] fp32 tensor --, then
//             F.cross_entropy, which writes a log-softmax of the same size, and autograd walks both back),
//             semantic_seg.py:241-243 (the same upsampling at inference) and
//             detectron2/modeling/postprocessing.py:77-100 (sem_seg_postprocess: crop + a second bilinear resize) with the
//             caller's argmax(dim=0).
// The geometry.  For an integer scale s, the full-res pixel Y = s b + s / 2 + j (0 <= j < s) reads the low-res rows b and
// b + 1 with the weights 1 - t_j and t_j, t_j = (j + 1/2) / s: exact in binary, the same s phases in every BLOCK b of
// s x s pixels "between four low-res centres".  b runs from -1 to h - 1; torch's border rule equals a replicate halo of
// one low-res pixel (the clamped row -1 is row 0, the clamped row h is row h - 1), and only the pixels of a border block
// that lie inside the image exist.  Below, blocks are counted from 0: block bb = b + 1 has the taps bb - 1 and bb.
// Here:
//   * a workgroup owns a TILE of 16 x tuy UNITS; a unit is a U x U piece of a block (U = min(s, 4): the whole block for
//     s = 2 and 4, a quarter of it for s = 8) and belongs to one thread: at most 16 full-res pixels live in its registers.
//     The low-res footprint of the tile -- its blocks plus one row and one column -- is staged ONCE in LDS as fp32
//     [class][row][col], from NCHW or channels_last input alike (the staging loop runs over the input's fastest axis).
//     tuy in {16, 8, 4} is picked by C: the largest with tile + slab <= 80 KB (two workgroups per CU), else the largest
//     that fits 160 KB: C = 54 -> 17 x 17 pixels, 62 KB; C = 256 -> 17 x 9 pixels, 157 KB (forward).
//   * loss forward: per class 4 LDS reads give the unit's U x U interpolated values (2 U + U U FMAs); a first pass over the
//     classes takes each pixel's maximum, a second the sum of exp(v - max) (one exp per value, no rescaling; exact
//     whatever the spread of the logits).  The target's logit is interpolated once per pixel from its own class.
//     lse goes to the workspace (4 B per full-res pixel), the unit's loss and counts into a fixed-order reduction:
//     butterfly per wave, waves in order, one record per workgroup, and a second one-workgroup launch adds the records in
//     fp64 in a fixed order.  No atomics: two runs are bit-identical.
//   * loss backward, a deterministic gather: the tile's blocks overlap the neighbour's by one (an edge block is computed
//     by both); per class a thread reduces its unit's (softmax - onehot) to the contributions to its block's four corners
//     with the constant weights and writes them to an LDS slab (two classes per barrier, double-buffered); then a thread
//     per low-res pixel adds its four blocks' contributions in a fixed order -- halo contributions are folded onto the
//     border pixel by the thread that made them -- and writes the sum INTO THE STAGED TILE, over the logit of the same
//     class, which nobody reads any more.  At the end the tile is the gradient and leaves the way the logits came in:
//     every element written exactly once, no zero fill.
//   * label decode: a workgroup owns 16 x 16 output pixels.  The two bilinear maps compose to at most 3 x 3 low-res taps
//     per output pixel (the two full-res taps are neighbours: they share a block or sit in adjacent ones); the low-res
//     footprint of the tile is staged in LDS in chunks of as many classes as fit, the argmax runs over the classes in
//     registers (strictly greater: the lowest class wins ties).  Nothing at full resolution is written.
//   MFMA does not fit: no contraction anywhere, every value is used once.
// Bound: VALU -- ~10 lane operations per (class, full-res pixel) in the forward -- not HBM: the compulsory
// bytes are logits + targets + lse (+ the gradient).
#include <algorithm>

#include "common.h"

namespace d2amd {

constexpr int SS_TW = 16;                 // units (threads) per tile row
constexpr int SS_MAX_C = 256;
constexpr int SS_LDS_MAX = 160 * 1024;    // LDS of a CU
constexpr int SS_LDS_PAIR = 80 * 1024;    // two workgroups per CU up to here
constexpr int SS_LDS_STATIC = 1024;       // kept free for the kernels' static arrays
constexpr int SS_CC = 2;                  // classes per slab of the backward
constexpr int SS_LT = 16;                 // side of the label decode's output tile

struct SsHeader { int64_t count; int64_t pad; };          // head of the workspace; then the records, then lse
struct SsPartial { double loss; int count; int oob; };    // one per workgroup of the forward

template <int S> struct ss_geom {
  static constexpr int U = S < 4 ? S : 4;  // side of a unit, full-res pixels
  static constexpr int Q = S / U;          // units per block side
};

// Stage the classes [c0, c0 + cc) of the low-res pixels [ly0, ly0 + PH) x [lx0, lx0 + PW), clamped to the image (the
// replicate halo; rows of a tile that hangs over the image repeat the last one), as fp32 tile[class - c0][row][col].
template <typename T>
__device__ __forceinline__ void ss_stage(const T* __restrict__ img, int C, int h, int w, int layout, int c0, int cc,
                                         int ly0, int lx0, int PH, int PW, float* __restrict__ tile, int tid, int nt) {
  const int P = PH * PW, total = cc * P;
  for (int idx = tid; idx < total; idx += nt) {
    int c, pix;
    if (layout == D2AMD_NHWC) { pix = idx / cc; c = idx - pix * cc; } else { c = idx / P; pix = idx - c * P; }
    const int py = pix / PW, px = pix - py * PW;
    const int y = min(max(ly0 + py, 0), h - 1), x = min(max(lx0 + px, 0), w - 1);
    const long at = layout == D2AMD_NHWC ? ((long)y * w + x) * C + (c0 + c) : ((long)(c0 + c) * h + y) * w + x;
    tile[c * P + pix] = to_f32(img[at]);
  }
}

// the U x U values of a unit from its block's four corners p[0], p[1], p[PW], p[PW + 1]
template <int U>
__device__ __forceinline__ void ss_interp(const float* __restrict__ p, int PW, const float (&wx)[U], const float (&wy)[U],
                                          float (&v)[U][U]) {
  const float a00 = p[0], a01 = p[1], a10 = p[PW], a11 = p[PW + 1];
  const float d0 = a01 - a00, d1 = a11 - a10;
  float top[U], dif[U];
#pragma unroll
  for (int j = 0; j < U; j++) {
    top[j] = fmaf(wx[j], d0, a00);
    dif[j] = fmaf(wx[j], d1, a10) - top[j];
  }
#pragma unroll
  for (int i = 0; i < U; i++)
#pragma unroll
    for (int j = 0; j < U; j++) v[i][j] = fmaf(wy[i], dif[j], top[j]);
}
__device__ __forceinline__ float ss_interp1(const float* __restrict__ p, int PW, float wx, float wy) {
  const float a00 = p[0], a01 = p[1], a10 = p[PW], a11 = p[PW + 1];
  const float top = fmaf(wx, a01 - a00, a00);
  return fmaf(wy, fmaf(wx, a11 - a10, a10) - top, top);
}

// What a thread knows of its unit.  Tile (blockIdx.x, blockIdx.y) starts at the block (bb0y, bb0x); LDS row / column r
// holds the low-res pixel bb0 - 1 + r.
template <int S> struct SsUnit {
  static constexpr int U = ss_geom<S>::U, Q = ss_geom<S>::Q;
  int corner;        // LDS offset of the block's top-left tap inside a class plane
  int bbx, bby;      // the block
  int X0, Y0;        // full-res coordinates of the unit's first pixel (negative in the halo)
  float wx[U], wy[U];
  __device__ __forceinline__ SsUnit(int tid, int bb0x, int bb0y, int PW) {
    const int tx = tid & (SS_TW - 1), ty = tid / SS_TW;
    const int cx = tx / Q, cy = ty / Q, j0x = (tx - cx * Q) * U, j0y = (ty - cy * Q) * U;
    corner = cy * PW + cx;
    bbx = bb0x + cx; bby = bb0y + cy;
    X0 = bbx * S - S / 2 + j0x;  // block bb covers the pixels S (bb - 1) + S / 2 + [0, S)
    Y0 = bby * S - S / 2 + j0y;
#pragma unroll
    for (int j = 0; j < U; j++) {
      wx[j] = ((float)(j0x + j) + 0.5f) * (1.f / (float)S);
      wy[j] = ((float)(j0y + j) + 0.5f) * (1.f / (float)S);
    }
  }
};

// The unit's targets: class in [0, C), or -1 for a pixel that does not count (outside the image, ignore_value, or a
// class outside [0, C), which is counted in `oob`).
template <int U>
__device__ __forceinline__ void ss_load_targets(const int64_t* __restrict__ tgt, int X0, int Y0, int SH, int SW, int C,
                                                int64_t ignore_value, int (&cls)[U][U], int& oob) {
#pragma unroll
  for (int i = 0; i < U; i++)
#pragma unroll
    for (int j = 0; j < U; j++) {
      const int Y = Y0 + i, X = X0 + j;
      const bool in = (unsigned)Y < (unsigned)SH && (unsigned)X < (unsigned)SW;
      const int64_t t = in ? tgt[(long)Y * SW + X] : ignore_value;
      const bool ign = t == ignore_value, bad = !ign && (t < 0 || t >= C);
      oob += bad;
      cls[i][j] = (ign || bad) ? -1 : (int)t;
    }
}

// ---- loss forward (semantic_seg.py:255-267) -------------------------------------------------------------------------
template <typename T, int S>
__global__ __launch_bounds__(256) void d2amd_sem_seg_loss_fwd_kernel(const T* __restrict__ logits,
                                                                     const int64_t* __restrict__ targets, int C, int h,
                                                                     int w, int layout, int tuy, int64_t ignore_value,
                                                                     float* __restrict__ lse_out,
                                                                     SsPartial* __restrict__ partials) {
  constexpr int U = ss_geom<S>::U, Q = ss_geom<S>::Q;
  extern __shared__ __attribute__((aligned(16))) float ss_tile[];
  __shared__ double sloss[4];
  __shared__ int scnt[4], soob[4];
  const int tid = threadIdx.x, nt = SS_TW * tuy;
  const int bxn = SS_TW / Q, byn = tuy / Q, PW = bxn + 1, PH = byn + 1, P = PW * PH;
  const int bb0x = blockIdx.x * bxn, bb0y = blockIdx.y * byn, n = blockIdx.z;
  const int SH = S * h, SW = S * w;
  ss_stage(logits + (long)n * C * h * w, C, h, w, layout, 0, C, bb0y - 1, bb0x - 1, PH, PW, ss_tile, tid, nt);
  const SsUnit<S> u(tid, bb0x, bb0y, PW);
  int cls[U][U], oob = 0;
  ss_load_targets<U>(targets + (long)n * SH * SW, u.X0, u.Y0, SH, SW, C, ignore_value, cls, oob);
  __syncthreads();

  const float* base = ss_tile + u.corner;
  float m[U][U], sum[U][U], v[U][U];
#pragma unroll
  for (int i = 0; i < U; i++)
#pragma unroll
    for (int j = 0; j < U; j++) { m[i][j] = -INFINITY; sum[i][j] = 0.f; }
  for (int c = 0; c < C; c++) {
    ss_interp<U>(base + c * P, PW, u.wx, u.wy, v);
#pragma unroll
    for (int i = 0; i < U; i++)
#pragma unroll
      for (int j = 0; j < U; j++) m[i][j] = fmaxf(m[i][j], v[i][j]);
  }
  for (int c = 0; c < C; c++) {
    ss_interp<U>(base + c * P, PW, u.wx, u.wy, v);  // (the same bits as in the first pass: v - m <= 0)
#pragma unroll
    for (int i = 0; i < U; i++)
#pragma unroll
      for (int j = 0; j < U; j++) sum[i][j] += __expf(v[i][j] - m[i][j]);
  }
  float loss = 0.f;
  int cnt = 0;
  float* lse_img = lse_out + (long)n * SH * SW;
#pragma unroll
  for (int i = 0; i < U; i++)
#pragma unroll
    for (int j = 0; j < U; j++) {
      const int Y = u.Y0 + i, X = u.X0 + j;
      const float lse = m[i][j] + logf(sum[i][j]);
      if ((unsigned)Y < (unsigned)SH && (unsigned)X < (unsigned)SW) lse_img[(long)Y * SW + X] = lse;
      if (cls[i][j] >= 0) {
        loss += lse - ss_interp1(base + cls[i][j] * P, PW, u.wx[j], u.wy[i]);
        cnt++;
      }
    }
  // fixed order: butterfly inside the wave, then the waves in order
  double dl = (double)loss;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    dl += __shfl_xor(dl, o, 64);
    cnt += __shfl_xor(cnt, o, 64);
    oob += __shfl_xor(oob, o, 64);
  }
  if ((tid & 63) == 0) { sloss[tid >> 6] = dl; scnt[tid >> 6] = cnt; soob[tid >> 6] = oob; }
  __syncthreads();
  if (tid == 0) {
    SsPartial r{0., 0, 0};
    for (int q = 0; q < nt / 64; q++) { r.loss += sloss[q]; r.count += scnt[q]; r.oob += soob[q]; }
    partials[((long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = r;
  }
}

__global__ __launch_bounds__(256) void d2amd_sem_seg_loss_final_kernel(const SsPartial* __restrict__ partials, int n,
                                                                       SsHeader* __restrict__ head,
                                                                       float* __restrict__ loss_out,
                                                                       int64_t* __restrict__ stats_out) {
  const int tid = threadIdx.x;
  double loss = 0.;
  long cnt = 0, oob = 0;
  for (int i = tid; i < n; i += 256) {
    loss += partials[i].loss;
    cnt += partials[i].count;
    oob += partials[i].oob;
  }
  __shared__ double sl[256];
  __shared__ long sc[256], so[256];
  sl[tid] = loss; sc[tid] = cnt; so[tid] = oob;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {  // fixed tree: deterministic
    if (tid < s) { sl[tid] += sl[tid + s]; sc[tid] += sc[tid + s]; so[tid] += so[tid + s]; }
    __syncthreads();
  }
  if (tid == 0) {
    *loss_out = (float)(sl[0] / (double)sc[0]);  // nothing counts: 0 / 0 = NaN, as torch's mean over no element
    stats_out[0] = sc[0];
    stats_out[1] = so[0];
    head->count = sc[0];
    head->pad = 0;
  }
}

// ---- loss backward --------------------------------------------------------------------------------------------------
// Tiles step by one block less than they hold: the output pixels of a tile are the low-res pixels bb0 .. bb0 + bn - 2,
// whose four blocks (bb and bb + 1 in each direction) are all inside it.
template <typename T, int S>
__global__ __launch_bounds__(256) void d2amd_sem_seg_loss_bwd_kernel(const T* __restrict__ logits,
                                                                     const int64_t* __restrict__ targets,
                                                                     const SsHeader* __restrict__ head,
                                                                     const float* __restrict__ lse_in,
                                                                     const float* __restrict__ grad_loss, int C, int h,
                                                                     int w, int layout, int tuy, int64_t ignore_value,
                                                                     T* __restrict__ grad) {
  constexpr int U = ss_geom<S>::U, Q = ss_geom<S>::Q;
  extern __shared__ __attribute__((aligned(16))) float ss_smem[];
  const int tid = threadIdx.x, nt = SS_TW * tuy;
  const int bxn = SS_TW / Q, byn = tuy / Q, PW = bxn + 1, PH = byn + 1, P = PW * PH;
  const int OX = bxn - 1, OY = byn - 1;
  float4* slab = reinterpret_cast<float4*>(ss_smem);  // [2][SS_CC][nt]: (g00, g01, g10, g11) of a unit
  float* ss_tile = ss_smem + 2 * SS_CC * nt * 4;      // [C][PH][PW] behind it
  const int bb0x = blockIdx.x * OX, bb0y = blockIdx.y * OY, n = blockIdx.z;
  const int SH = S * h, SW = S * w;
  ss_stage(logits + (long)n * C * h * w, C, h, w, layout, 0, C, bb0y - 1, bb0x - 1, PH, PW, ss_tile, tid, nt);
  const SsUnit<S> u(tid, bb0x, bb0y, PW);
  int cls[U][U], oob = 0;
  ss_load_targets<U>(targets + (long)n * SH * SW, u.X0, u.Y0, SH, SW, C, ignore_value, cls, oob);
  // lse = +inf where the pixel does not count: exp(v - inf) = 0 and its class (-1) matches nothing
  float lse[U][U];
  const float* lse_img = lse_in + (long)n * SH * SW;
#pragma unroll
  for (int i = 0; i < U; i++)
#pragma unroll
    for (int j = 0; j < U; j++) lse[i][j] = cls[i][j] >= 0 ? lse_img[(long)(u.Y0 + i) * SW + (u.X0 + j)] : INFINITY;
  const long count = head->count;
  const float scale = count > 0 ? *grad_loss / (float)count : 0.f;
  // a border block has both taps on the border pixel: its halo half is folded onto the other one here
  const bool fold_l = u.bbx == 0, fold_r = u.bbx == w, fold_t = u.bby == 0, fold_b = u.bby == h;
  __syncthreads();

  const float* base = ss_tile + u.corner;
  const int per_chunk = OY * OX;
  for (int c0 = 0, k = 0; c0 < C; c0 += SS_CC, k ^= 1) {
    float4* sl = slab + (size_t)k * SS_CC * nt;
#pragma unroll
    for (int q = 0; q < SS_CC; q++) {
      const int c = c0 + q;
      if (c < C) {
        float v[U][U];
        ss_interp<U>(base + c * P, PW, u.wx, u.wy, v);
        float g00 = 0.f, g01 = 0.f, g10 = 0.f, g11 = 0.f;
#pragma unroll
        for (int i = 0; i < U; i++) {
          float r0 = 0.f, r1 = 0.f;
#pragma unroll
          for (int j = 0; j < U; j++) {
            const float e = __expf(v[i][j] - lse[i][j]) - (cls[i][j] == c ? 1.f : 0.f);
            r0 = fmaf(1.f - u.wx[j], e, r0);
            r1 = fmaf(u.wx[j], e, r1);
          }
          g00 = fmaf(1.f - u.wy[i], r0, g00); g01 = fmaf(1.f - u.wy[i], r1, g01);
          g10 = fmaf(u.wy[i], r0, g10); g11 = fmaf(u.wy[i], r1, g11);
        }
        if (fold_l) { g01 += g00; g11 += g10; g00 = 0.f; g10 = 0.f; }
        if (fold_r) { g00 += g01; g10 += g11; g01 = 0.f; g11 = 0.f; }
        if (fold_t) { g10 += g00; g11 += g01; g00 = 0.f; g01 = 0.f; }
        if (fold_b) { g00 += g10; g01 += g11; g10 = 0.f; g11 = 0.f; }
        sl[q * nt + tid] = make_float4(g00, g01, g10, g11);
      }
    }
    __syncthreads();  // (one barrier per chunk: the next chunk writes the other slab, and other classes of the tile)
    const int todo = min(SS_CC, C - c0) * per_chunk;
    for (int idx = tid; idx < todo; idx += nt) {
      const int q = idx / per_chunk, o = idx - q * per_chunk;
      const int oy = o / OX, ox = o - oy * OX;
      const float* s = reinterpret_cast<const float*>(sl + q * nt);
      float acc = 0.f;
      // pixel (oy, ox) is the corner (1 - dy, 1 - dx) of the block (oy + dy, ox + dx): a fixed order of blocks and units
#pragma unroll
      for (int dy = 0; dy < 2; dy++)
#pragma unroll
        for (int dx = 0; dx < 2; dx++)
#pragma unroll
          for (int qy = 0; qy < Q; qy++)
#pragma unroll
            for (int qx = 0; qx < Q; qx++)
              acc += s[(((oy + dy) * Q + qy) * SS_TW + (ox + dx) * Q + qx) * 4 + (1 - dy) * 2 + (1 - dx)];
      ss_tile[(c0 + q) * P + (oy + 1) * PW + ox + 1] = acc * scale;  // over the logit nobody reads any more
    }
  }
  __syncthreads();
  // the tile is the gradient now: out the way it came in
  T* gimg = grad + (long)n * C * h * w;
  const int total = C * per_chunk;
  for (int idx = tid; idx < total; idx += nt) {
    int c, o;
    if (layout == D2AMD_NHWC) { o = idx / C; c = idx - o * C; } else { c = idx / per_chunk; o = idx - c * per_chunk; }
    const int oy = o / OX, ox = o - oy * OX;
    const int y = bb0y + oy, x = bb0x + ox;
    if (y < h && x < w) {
      const long at = layout == D2AMD_NHWC ? ((long)y * w + x) * C + c : ((long)c * h + y) * w + x;
      gimg[at] = from_f32<T>(ss_tile[c * P + (oy + 1) * PW + ox + 1]);
    }
  }
}

// ---- label decode (semantic_seg.py:241-243 + postprocessing.py:77-100 + argmax) ---------------------------------------
// Output coordinate o of the second resize (`in` cropped full-res pixels -> `out`, torch's align_corners=False rule with
// scale = in / out) composed with the first: the low-res rows r0, r0 + 1, r0 + 2 (not yet clamped) with the weights wt.
template <int S>
__device__ __forceinline__ void ss_label_taps(int o, int in, float sc, int& r0, float (&wt)[3]) {
  const float src = fmaxf(sc * ((float)o + 0.5f) - 0.5f, 0.f);
  const int Y0 = min((int)src, in - 1);
  const int Y1 = Y0 + (Y0 < in - 1 ? 1 : 0);
  const float lam = fminf(src - (float)Y0, 1.f);
  const int b0 = (Y0 + S / 2) / S, b1 = (Y1 + S / 2) / S;  // the full-res pixel Y lies in block (Y + S / 2) / S
  const float t0 = ((float)(Y0 + S / 2 - b0 * S) + 0.5f) * (1.f / (float)S);
  const float t1 = ((float)(Y1 + S / 2 - b1 * S) + 0.5f) * (1.f / (float)S);
  r0 = b0 - 1;
  wt[0] = (1.f - lam) * (1.f - t0);
  wt[1] = (1.f - lam) * t0;
  wt[2] = 0.f;
  if (b1 == b0) {
    wt[0] = fmaf(lam, 1.f - t1, wt[0]);
    wt[1] = fmaf(lam, t1, wt[1]);
  } else {
    wt[1] = fmaf(lam, 1.f - t1, wt[1]);
    wt[2] = lam * t1;
  }
}

template <typename T, int S>
__global__ __launch_bounds__(SS_LT * SS_LT) void d2amd_sem_seg_labels_kernel(const T* __restrict__ logits, int C, int h,
                                                                             int w, int layout, int ih, int iw, int oh,
                                                                             int ow, float sy, float sx, int lds_floats,
                                                                             int64_t* __restrict__ labels) {
  extern __shared__ __attribute__((aligned(16))) float ss_tile[];
  constexpr int NT = SS_LT * SS_LT;
  const int tid = threadIdx.x, n = blockIdx.z;
  const int ox0 = blockIdx.x * SS_LT, oy0 = blockIdx.y * SS_LT;
  const int ox = ox0 + (tid & (SS_LT - 1)), oy = oy0 + tid / SS_LT;
  // the tile's low-res footprint: the taps are monotonic in the output coordinate
  int r_first, r_last, q_first, q_last, ry, rx;
  float wy[3], wx[3];
  ss_label_taps<S>(oy0, ih, sy, r_first, wy);
  ss_label_taps<S>(min(oy0 + SS_LT, oh) - 1, ih, sy, r_last, wy);
  ss_label_taps<S>(ox0, iw, sx, q_first, wx);
  ss_label_taps<S>(min(ox0 + SS_LT, ow) - 1, iw, sx, q_last, wx);
  const int ylo = min(max(r_first, 0), h - 1), yhi = min(max(r_last + 2, 0), h - 1);
  const int xlo = min(max(q_first, 0), w - 1), xhi = min(max(q_last + 2, 0), w - 1);
  const int FH = yhi - ylo + 1, FW = xhi - xlo + 1, P = FH * FW;
  ss_label_taps<S>(min(oy, oh - 1), ih, sy, ry, wy);  // (threads behind the image repeat its last pixel and store nothing)
  ss_label_taps<S>(min(ox, ow - 1), iw, sx, rx, wx);
  const bool live = oy < oh && ox < ow;
  int64_t* out = labels + ((long)n * oh + oy) * ow + ox;
  const int cc = min(C, lds_floats / P);
  if (cc < 1) {  // (the host sized the LDS for a footprint at least this large: not reached)
    if (live) *out = -1;
    return;
  }
  int ro[3], co[3];
#pragma unroll
  for (int a = 0; a < 3; a++) {
    ro[a] = (min(max(ry + a, ylo), yhi) - ylo) * FW;
    co[a] = min(max(rx + a, xlo), xhi) - xlo;
  }
  const T* img = logits + (long)n * C * h * w;
  float best = -INFINITY;
  int bc = 0;
  for (int c0 = 0; c0 < C; c0 += cc) {
    const int nc = min(cc, C - c0);
    if (c0) __syncthreads();  // the previous chunk has been read
    ss_stage(img, C, h, w, layout, c0, nc, ylo, xlo, FH, FW, ss_tile, tid, NT);
    __syncthreads();
    for (int c = 0; c < nc; c++) {
      const float* p = ss_tile + c * P;
      float v = 0.f;
#pragma unroll
      for (int a = 0; a < 3; a++) {
        const float* row = p + ro[a];
        float r = wx[0] * row[co[0]];
        r = fmaf(wx[1], row[co[1]], r);
        r = fmaf(wx[2], row[co[2]], r);
        v = fmaf(wy[a], r, v);
      }
      const bool take = v > best;  // strictly: the lowest class wins ties
      best = take ? v : best;
      bc = take ? c0 + c : bc;
    }
  }
  if (live) *out = bc;
}

// ---- host ------------------------------------------------------------------------------------------------------------
struct SsPlan { int tuy; int tiles_x, tiles_y; size_t lds; };

// tile of the loss kernels: the largest tuy whose LDS (tile + the backward's slab) lets two workgroups share a CU, else
// the largest that fits at all; tuy = 0: none (not reached for C <= 256)
static SsPlan ss_plan(int C, int h, int w, int S, bool backward) {
  const int Q = S / (S < 4 ? S : 4);
  const int budgets[2] = {SS_LDS_PAIR, SS_LDS_MAX};
  SsPlan p{0, 0, 0, 0};
  for (int b = 0; b < 2 && !p.tuy; b++)
    for (int tuy = 16; tuy >= 4 && !p.tuy; tuy >>= 1) {
      const int bxn = SS_TW / Q, byn = tuy / Q;
      const size_t lds = (size_t)C * (bxn + 1) * (byn + 1) * 4 + (backward ? (size_t)2 * SS_CC * SS_TW * tuy * 16 : 0);
      if (lds + SS_LDS_STATIC > (size_t)budgets[b]) continue;
      p.tuy = tuy;
      p.lds = lds;
      // forward: the blocks 0 .. w (w + 1 of them) in steps of bxn; backward: the pixels 0 .. w - 1 in steps of bxn - 1
      p.tiles_x = backward ? cdiv(w, bxn - 1) : cdiv(w + 1, bxn);
      p.tiles_y = backward ? cdiv(h, byn - 1) : cdiv(h + 1, byn);
    }
  return p;
}

static size_t ss_max_partials(int N, int h, int w, int S) {  // the smallest tile (tuy = 4) makes the most workgroups
  const int Q = S / (S < 4 ? S : 4);
  return (size_t)N * cdiv(w + 1, SS_TW / Q) * cdiv(h + 1, 4 / Q);
}

}  // namespace d2amd

using namespace d2amd;

#define SS_CHECK_COMMON(op)                                                                                           \
  do {                                                                                                                \
    D2_CHECK_ARG(N >= 0 && C >= 1 && h >= 1 && w >= 1, op ": bad shape");                                             \
    if (!(s == 2 || s == 4 || s == 8) || C > SS_MAX_C || (layout != D2AMD_NCHW && layout != D2AMD_NHWC) ||            \
        (dtype != D2AMD_F32 && dtype != D2AMD_F16 && dtype != D2AMD_BF16)) {                                          \
      ::d2amd::set_error(op ": scale %d / %d classes / layout %d / dtype %d not supported (scale 2, 4 or 8, <= %d "   \
                         "classes, NCHW or NHWC, fp32 / f16 / bf16)", s, C, layout, dtype, SS_MAX_C);                 \
      return D2AMD_EUNSUPPORTED;                                                                                      \
    }                                                                                                                 \
    D2_CHECK_ARG((long)N * C * h * w < (1l << 31) && (long)N * s * h * s * w < (1l << 31) && N < 65536,               \
                 op ": tensor too large");                                                                            \
  } while (0)

#define SS_DISPATCH_SCALE(s, ...)                                \
  [&]() -> int {                                                 \
    switch (s) {                                                 \
      case 2: { constexpr int S = 2; return __VA_ARGS__(); }     \
      case 4: { constexpr int S = 4; return __VA_ARGS__(); }     \
      default: { constexpr int S = 8; return __VA_ARGS__(); }    \
    }                                                            \
  }()

extern "C" size_t d2amd_sem_seg_loss_workspace_bytes(int N, int h, int w, int s) {
  if (N < 1 || h < 1 || w < 1 || !(s == 2 || s == 4 || s == 8)) return sizeof(SsHeader);
  return sizeof(SsHeader) + ss_max_partials(N, h, w, s) * sizeof(SsPartial) + (size_t)N * s * h * s * w * 4;
}

extern "C" int d2amd_sem_seg_loss_forward(const void* logits, const int64_t* targets, int N, int C, int h, int w, int s,
                                          int dtype, int layout, int64_t ignore_value, float* loss_out,
                                          int64_t* stats_out, void* workspace, size_t workspace_bytes, void* stream) {
  SS_CHECK_COMMON("sem_seg_loss_forward");
  D2_CHECK_ARG(N > 0, "sem_seg_loss_forward: empty batch");
  D2_CHECK_ARG(logits && targets && loss_out && stats_out, "sem_seg_loss_forward: null pointer");
  D2_CHECK_ARG(workspace && ((uintptr_t)workspace & 7) == 0 &&
                   workspace_bytes >= d2amd_sem_seg_loss_workspace_bytes(N, h, w, s),
               "sem_seg_loss_forward: workspace too small or misaligned (%zu bytes, %zu needed)", workspace_bytes,
               d2amd_sem_seg_loss_workspace_bytes(N, h, w, s));
  const SsPlan p = ss_plan(C, h, w, s, false);
  D2_CHECK_ARG(p.tuy > 0 && p.tiles_y < 65536, "sem_seg_loss_forward: no tile for this shape");
  SsHeader* head = (SsHeader*)workspace;
  SsPartial* partials = (SsPartial*)(head + 1);
  float* lse = (float*)(partials + ss_max_partials(N, h, w, s));
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(p.tiles_x, p.tiles_y, N);
  const int nwg = p.tiles_x * p.tiles_y * N;
  return D2_DISPATCH_DTYPE(dtype, [&]() -> int {
    return SS_DISPATCH_SCALE(s, [&]() -> int {
      auto kern = d2amd_sem_seg_loss_fwd_kernel<scalar_t, S>;
      if (p.lds > 64 * 1024)
        D2_HIP_OK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds));
      hipLaunchKernelGGL(kern, grid, dim3(SS_TW * p.tuy), p.lds, st, (const scalar_t*)logits, targets, C, h, w, layout,
                         p.tuy, ignore_value, lse, partials);
      D2_LAUNCH_OK();
      hipLaunchKernelGGL(d2amd_sem_seg_loss_final_kernel, dim3(1), dim3(256), 0, st, partials, nwg, head, loss_out,
                         stats_out);
      D2_LAUNCH_OK();
      return D2AMD_OK;
    });
  });
}

extern "C" int d2amd_sem_seg_loss_backward(const void* logits, const int64_t* targets, const void* workspace,
                                           const float* grad_loss, int N, int C, int h, int w, int s, int dtype,
                                           int layout, int64_t ignore_value, void* grad_logits, void* stream) {
  SS_CHECK_COMMON("sem_seg_loss_backward");
  D2_CHECK_ARG(N > 0, "sem_seg_loss_backward: empty batch");
  D2_CHECK_ARG(logits && targets && workspace && grad_loss && grad_logits, "sem_seg_loss_backward: null pointer");
  const SsPlan p = ss_plan(C, h, w, s, true);
  D2_CHECK_ARG(p.tuy > 0 && p.tiles_y < 65536, "sem_seg_loss_backward: no tile for this shape");
  const SsHeader* head = (const SsHeader*)workspace;
  const SsPartial* partials = (const SsPartial*)(head + 1);
  const float* lse = (const float*)(partials + ss_max_partials(N, h, w, s));
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(p.tiles_x, p.tiles_y, N);
  return D2_DISPATCH_DTYPE(dtype, [&]() -> int {
    return SS_DISPATCH_SCALE(s, [&]() -> int {
      auto kern = d2amd_sem_seg_loss_bwd_kernel<scalar_t, S>;
      if (p.lds > 64 * 1024)
        D2_HIP_OK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds));
      hipLaunchKernelGGL(kern, grid, dim3(SS_TW * p.tuy), p.lds, st, (const scalar_t*)logits, targets, head, lse,
                         grad_loss, C, h, w, layout, p.tuy, ignore_value, (scalar_t*)grad_logits);
      D2_LAUNCH_OK();
      return D2AMD_OK;
    });
  });
}

extern "C" int d2amd_sem_seg_labels(const void* logits, int N, int C, int h, int w, int s, int dtype, int layout, int ih,
                                    int iw, int oh, int ow, int64_t* labels, void* stream) {
  SS_CHECK_COMMON("sem_seg_labels");
  D2_CHECK_ARG(ih >= 1 && iw >= 1 && ih <= s * h && iw <= s * w, "sem_seg_labels: image size (%d, %d) outside (%d, %d)",
               ih, iw, s * h, s * w);
  D2_CHECK_ARG(oh >= 1 && ow >= 1 && (long)N * oh * ow < (1l << 31), "sem_seg_labels: bad output size (%d, %d)", oh, ow);
  if (N == 0) return D2AMD_OK;
  D2_CHECK_ARG(logits && labels, "sem_seg_labels: null pointer");
  const float sy = (float)((double)ih / oh), sx = (float)((double)iw / ow);
  // rows of a tile's footprint: its 16 outputs span <= floor(15 sy) + 1 full-res rows, those <= floor(15 sy / s) + 1
  // more blocks, a block's taps 2 rows and the last output's taps one more (+ 2 against the rounding of sy)
  const long fh = std::min<long>(h, (long)(sy * (SS_LT - 1) / s) + 6), fw = std::min<long>(w, (long)(sx * (SS_LT - 1) / s) + 6);
  const size_t one = (size_t)fh * fw * 4;
  if (one + SS_LDS_STATIC > (size_t)SS_LDS_MAX) {
    ::d2amd::set_error("sem_seg_labels: downscaling (%d, %d) -> (%d, %d) needs a %ld x %ld footprint per tile", ih, iw,
                       oh, ow, fh, fw);
    return D2AMD_EUNSUPPORTED;
  }
  const size_t lds = std::min<size_t>(one * C, std::max<size_t>(one, 64 * 1024));
  const dim3 grid(cdiv(ow, SS_LT), cdiv(oh, SS_LT), N);
  D2_CHECK_ARG(grid.y < 65536, "sem_seg_labels: output too tall");
  hipStream_t st = (hipStream_t)stream;
  return D2_DISPATCH_DTYPE(dtype, [&]() -> int {
    return SS_DISPATCH_SCALE(s, [&]() -> int {
      auto kern = d2amd_sem_seg_labels_kernel<scalar_t, S>;
      if (lds > 64 * 1024)
        D2_HIP_OK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      hipLaunchKernelGGL(kern, grid, dim3(SS_LT * SS_LT), lds, st, (const scalar_t*)logits, C, h, w, layout, ih, iw, oh,
                         ow, sy, sx, (int)(lds / 4), labels);
      D2_LAUNCH_OK();
      return D2AMD_OK;
    });
  });
}
