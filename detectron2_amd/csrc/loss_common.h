// Pieces the fused training losses share (dense_loss.hip, box_loss.hip, fcos.hip): 16-byte vectors of the I/O dtype, the
// box regression term of one foreground row, GIoU on corners, the focal / BCE term, the wave butterfly.
#pragma once
#include "common.h"

namespace d2amd {

// ---- 16-byte vectors of T <-> fp32 ------------------------------------------------------------------------------
template <typename T> struct dl_vec { static constexpr int N = 16 / (int)sizeof(T); };

__device__ __forceinline__ void dl_load16(const float* p, float (&o)[4]) {
  const float4 v = *reinterpret_cast<const float4*>(p);
  o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
}
template <typename T> __device__ __forceinline__ void dl_load16(const T* p, float (&o)[8]) {
  const uint4 v = *reinterpret_cast<const uint4*>(p);
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int q = 0; q < 4; q++) {
    o[2 * q] = to_f32(T{(uint16_t)(w[q] & 0xffffu)});
    o[2 * q + 1] = to_f32(T{(uint16_t)(w[q] >> 16)});
  }
}
__device__ __forceinline__ void dl_store16(float* p, const float (&i)[4]) {
  *reinterpret_cast<float4*>(p) = make_float4(i[0], i[1], i[2], i[3]);
}
template <typename T> __device__ __forceinline__ void dl_store16(T* p, const float (&i)[8]) {
  uint32_t w[4];
#pragma unroll
  for (int q = 0; q < 4; q++)
    w[q] = (uint32_t)from_f32<T>(i[2 * q]).v | ((uint32_t)from_f32<T>(i[2 * q + 1]).v << 16);
  *reinterpret_cast<uint4*>(p) = uint4{w[0], w[1], w[2], w[3]};
}

// elements in front of the first 16-byte boundary at or behind p (all of them when `vec` is off)
template <typename T> __device__ __forceinline__ int dl_head(const T* p, int count, bool vec) {
  if (!vec) return count;
  const int h = (int)(((16u - (uint32_t)((uintptr_t)p & 15u)) & 15u) / (uint32_t)sizeof(T));
  return min(h, count);
}

// ---- box term of one foreground anchor (box_regression.py:43-116, fvcore smooth_l1_loss / giou_loss) -----------
// F: the type the geometry is computed in.  float is the dense-anchor losses' (hundreds of foreground anchors per
// tile); double is the box head's: get_deltas subtracts box centres of several hundred pixels, which in fp32 leaves
// 1e-5 of a delta (measured 2.7e-6 on grad * rows against float64), and a workgroup there has a handful of rows.
__device__ __forceinline__ float dl_log(float x) { return logf(x); }
__device__ __forceinline__ double dl_log(double x) { return log(x); }
__device__ __forceinline__ float dl_exp(float x) { return expf(x); }
__device__ __forceinline__ double dl_exp(double x) { return exp(x); }
__device__ __forceinline__ float dl_min(float a, float b) { return fminf(a, b); }
__device__ __forceinline__ double dl_min(double a, double b) { return fmin(a, b); }
__device__ __forceinline__ float dl_max(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ double dl_max(double a, double b) { return fmax(a, b); }
__device__ __forceinline__ float dl_abs(float x) { return fabsf(x); }
__device__ __forceinline__ double dl_abs(double x) { return fabs(x); }

// torch's rule for max / min of equal arguments: the gradient is shared
template <typename F> __device__ __forceinline__ F dl_sel_gt(F a, F b) { return a > b ? F(1) : (a == b ? F(0.5) : F(0)); }

// GIoU loss (fvcore giou_loss, eps 1e-7) of the corner box (x1, y1, x2, y2) against gt; g = d loss / d (x1, y1, x2, y2)
template <typename F>
__device__ __forceinline__ F dl_giou_corners(F x1, F y1, F x2, F y2, const float (&gt)[4], F (&g)[4]) {
  const F X1 = gt[0], Y1 = gt[1], X2 = gt[2], Y2 = gt[3];
  constexpr F eps = (F)1e-7;
  const F iw = dl_min(x2, X2) - dl_max(x1, X1), ih = dl_min(y2, Y2) - dl_max(y1, Y1);
  const bool hit = iw > F(0) && ih > F(0);
  const F I = hit ? iw * ih : F(0);
  const F bw = x2 - x1, bh = y2 - y1;
  const F U = bw * bh + (X2 - X1) * (Y2 - Y1) - I;
  const F cw = dl_max(x2, X2) - dl_min(x1, X1), ch = dl_max(y2, Y2) - dl_min(y1, Y1);
  const F C = cw * ch;
  const F iu = F(1) / (U + eps), ic = F(1) / (C + eps);
  const F loss = F(1) - I * iu + (C - U) * ic;
  // loss(I, U, C) with U = area_pred + area_gt - I
  const F gU = I * iu * iu - ic;
  const F gI = -iu - gU;
  const F gC = (U + eps) * ic * ic;
  const F hI = hit ? gI : F(0);
  g[0] = -gU * bh - hI * ih * dl_sel_gt(x1, X1) - gC * ch * dl_sel_gt(X1, x1);
  g[1] = -gU * bw - hI * iw * dl_sel_gt(y1, Y1) - gC * cw * dl_sel_gt(Y1, y1);
  g[2] = gU * bh + hI * ih * dl_sel_gt(X2, x2) + gC * ch * dl_sel_gt(x2, X2);
  g[3] = gU * bw + hI * iw * dl_sel_gt(Y2, y2) + gC * cw * dl_sel_gt(y2, Y2);
  return loss;
}

// -> loss; g[0..3] = d loss / d delta
// P: a parameter block with giou, beta, wx, wy, ww, wh, scale_clamp
template <typename F = float, typename P>
__device__ __forceinline__ float dl_box_term(const float (&an)[4], const float (&gt)[4], const float (&d)[4], const P& p,
                                             float (&g)[4]) {
  const F half = F(0.5), beta = p.beta, clamp = p.scale_clamp;
  const F w = (F)an[2] - (F)an[0], h = (F)an[3] - (F)an[1];
  const F cx = (F)an[0] + half * w, cy = (F)an[1] + half * h;
  if (!p.giou) {
    const F tw = (F)gt[2] - (F)gt[0], th = (F)gt[3] - (F)gt[1];
    const F tcx = (F)gt[0] + half * tw, tcy = (F)gt[1] + half * th;
    const F tgt[4] = {p.wx * (tcx - cx) / w, p.wy * (tcy - cy) / h, p.ww * dl_log(tw / w), p.wh * dl_log(th / h)};
    F loss = F(0);
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const F r = (F)d[i] - tgt[i], n = dl_abs(r);
      const F sgn = r > F(0) ? F(1) : (r < F(0) ? F(-1) : F(0));
      if (p.beta < 1e-5f || !(n < beta)) {
        loss += p.beta < 1e-5f ? n : n - half * beta;
        g[i] = (float)sgn;
      } else {
        loss += half * n * n / beta;
        g[i] = (float)(r / beta);
      }
    }
    return (float)loss;
  }
  // apply_deltas, then GIoU with eps = 1e-7
  const F dx = (F)d[0] / p.wx, dy = (F)d[1] / p.wy;
  const F dw0 = (F)d[2] / p.ww, dh0 = (F)d[3] / p.wh;
  const F dw = dl_min(dw0, clamp), dh = dl_min(dh0, clamp);
  const F pcx = dx * w + cx, pcy = dy * h + cy;
  const F pw = dl_exp(dw) * w, ph = dl_exp(dh) * h;
  F gc[4];
  const F loss = dl_giou_corners<F>(pcx - half * pw, pcy - half * ph, pcx + half * pw, pcy + half * ph, gt, gc);
  const F gx1 = gc[0], gy1 = gc[1], gx2 = gc[2], gy2 = gc[3];
  g[0] = (float)((gx1 + gx2) * w / p.wx);
  g[1] = (float)((gy1 + gy2) * h / p.wy);
  g[2] = dw0 > clamp ? 0.f : (float)(half * (gx2 - gx1) * pw / p.ww);  // a clamped delta has no gradient
  g[3] = dh0 > clamp ? 0.f : (float)(half * (gy2 - gy1) * ph / p.wh);
  return (float)loss;
}

// ---- focal / BCE term (fvcore sigmoid_focal_loss, F.binary_cross_entropy_with_logits) ---------------------------
// GM: 0 gamma == 0, 2 gamma == 2, 1 any other gamma > 0;  P: a parameter block with alpha, gamma
__device__ __forceinline__ float dl_alpha_t(bool t, float alpha) { return alpha >= 0.f ? (t ? alpha : 1.f - alpha) : 1.f; }

template <int GM, typename P> __device__ __forceinline__ float dl_focal(float x, int code, int c, const P& p) {
  const bool t = code == c;
  const float z = t ? -x : x;
  const float e = __expf(-fabsf(x));
  const float l = __logf(1.f + e);
  const float ce = fmaxf(z, 0.f) + l;
  float mod = 1.f;
  if (GM == 2) {
    const float s = __builtin_amdgcn_rcpf(1.f + e);
    const float q = z >= 0.f ? s : e * s;
    mod = q * q;
  } else if (GM == 1) {
    mod = __expf(-p.gamma * (fmaxf(-z, 0.f) + l));
  }
  const float v = dl_alpha_t(t, p.alpha) * ce * mod;
  return code < 0 ? 0.f : v;  // (a select: an ignored row's NaN stays out)
}

// d loss / d x, times the upstream gradient g
template <int GM, typename P>
__device__ __forceinline__ float dl_focal_grad(float x, int code, int c, const P& p, float g) {
  const bool t = code == c;
  const float z = t ? -x : x;
  const float e = __expf(-fabsf(x));
  const float s = __builtin_amdgcn_rcpf(1.f + e);
  const float q = z >= 0.f ? s : e * s, omq = z >= 0.f ? e * s : s;
  float d = q;
  if (GM != 0) {
    const float l = __logf(1.f + e);
    const float ce = fmaxf(z, 0.f) + l;
    const float mod = GM == 2 ? q * q : __expf(-p.gamma * (fmaxf(-z, 0.f) + l));
    d = mod * (q + p.gamma * ce * omq);
  }
  const float v = dl_alpha_t(t, p.alpha) * d * (t ? -g : g);
  return code < 0 ? 0.f : v;
}

__device__ __forceinline__ float dl_wave_sum(float v) {  // butterfly: every lane ends with the same bits
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

}  // namespace d2amd
