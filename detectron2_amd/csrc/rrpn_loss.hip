// Training losses of the rotated proposal generator, fused: objectness BCE + rotated box regression of ALL images and
// levels in one forward and one backward launch.
//   replaces  detectron2/modeling/proposal_generator/rpn.py:366-429 (RPN.losses as RRPN inherits it: cat of the per-level
//             logits and deltas, two boolean indices, two `.item()`s, autograd back through every copy) with
//             detectron2/modeling/box_regression.py:145-181 (Box2BoxTransformRotated.get_deltas over all N x R anchors,
//             then the foreground index) and fvcore's smooth_l1_loss.
// Here:
//   * a WORKGROUP (256 threads) OWNS A TILE of RL_TILE = 256 consecutive anchors of one (image, level); thread i owns
//     anchor i: label (int8), logit (K = 1: the tile's logits are 256 consecutive elements, one coalesced access) and,
//     where the label is 1, the five-column box term.  The level table is a by-value kernel argument.
//   * targets in the kernel, in fp64 (a tile has a handful of foreground rows; the centre differences of several hundred
//     pixels and the angle wrap stay exact):  dx = wx (tcx - cx) / w, dy = wy (tcy - cy) / h, dw = ww log(tw / w),
//     dh = wh log(th / h), da = wa pi / 180 (((ta - a + 180) mod 360) - 180) with the floor-mod of torch: a difference
//     of exactly +-180 degrees gives -180.
//   * forward: the foreground rows fetch their own delta row and anchor (sparse); butterfly inside a wave, four waves
//     added in order, one (cls, box, #fg, #valid) record per tile; a one-workgroup kernel adds the records in fp64 in a
//     fixed order.  No float atomics: bit-identical runs.
//   * backward: the tile's cnt x 5 delta gradients are CONTIGUOUS in memory but a row of five is no power of two: thread i
//     puts its row (zeros unless foreground) into LDS at 5 i (stride 5: conflict free), and the workgroup then stores the
//     cnt * 5 elements with consecutive lanes on consecutive addresses.  Every gradient element of every level is written
//     once, zeros included; the gradient is recomputed from the inputs, the forward saves nothing per element.
// LDS: 5 KB (backward), 32 B (forward).  Roofline: HBM -- per anchor 1 label byte + 1 logit read, 1 + 5 elements written.
#pragma clang fp contract(off)
#include "common.h"
#include "loss_common.h"

namespace d2amd {

constexpr int RL_TILE = 256;     // anchors per workgroup
constexpr int RL_THREADS = 256;  // == RL_TILE
constexpr int RL_MAX_LEVELS = D2AMD_RPN_MAX_LEVELS;

struct RlLevels {
  const void* logits[RL_MAX_LEVELS];   // [N, A_l]
  const void* deltas[RL_MAX_LEVELS];   // [N, A_l, 5]
  const float* anchors[RL_MAX_LEVELS]; // [A_l, 5]
  void* glogits[RL_MAX_LEVELS];        // backward only
  void* gdeltas[RL_MAX_LEVELS];
  int A[RL_MAX_LEVELS];
  int aoff[RL_MAX_LEVELS];             // prefix of A_l: the level's first column of gt_labels / gt_boxes
  int tile_base[RL_MAX_LEVELS + 1];    // prefix of N * cdiv(A_l, RL_TILE); entries behind L repeat the total
  int L;
};

struct RlParams {
  int N, R;
  float alpha, gamma;  // (-1, 0): what dl_focal<0> reads for plain BCE
  float beta, w[5];
};

struct RlPartial { float cls, box; int fg, valid; };  // one per tile

struct RlTile {
  const void* logits; const void* deltas; const float* anchors; void* glogits; void* gdeltas;
  int A, col0, n, a0, cnt;  // col0: column of anchor a0 in gt_labels / gt_boxes
};

__device__ __forceinline__ RlTile rl_tile(const RlLevels& P, int b) {
  int l = 0;
#pragma unroll
  for (int q = 1; q < RL_MAX_LEVELS; q++)
    if (q < P.L && b >= P.tile_base[q]) l = q;
  RlTile t{};
  int base = 0, aoff = 0;
#pragma unroll
  for (int q = 0; q < RL_MAX_LEVELS; q++)  // (selects: no runtime index into the by-value argument)
    if (q == l) {
      t.logits = P.logits[q]; t.deltas = P.deltas[q]; t.anchors = P.anchors[q];
      t.glogits = P.glogits[q]; t.gdeltas = P.gdeltas[q];
      t.A = P.A[q]; aoff = P.aoff[q]; base = P.tile_base[q];
    }
  const int per_image = (t.A + RL_TILE - 1) / RL_TILE;
  const int r = b - base;
  t.n = r / per_image;
  t.a0 = (r - t.n * per_image) * RL_TILE;
  t.cnt = min(RL_TILE, t.A - t.a0);
  t.col0 = aoff + t.a0;
  return t;
}

// label -> code for dl_focal (class 0 of K = 1): 0 foreground, 1 background, -1 ignored (any other value)
__device__ __forceinline__ int rl_code(const int8_t* __restrict__ gt_labels, const RlParams& p, const RlTile& t, int tid) {
  if (tid >= t.cnt) return -1;
  const int v = gt_labels[(long)t.n * p.R + t.col0 + tid];
  return v == 1 ? 0 : (v == 0 ? 1 : -1);
}

// box_regression.py:160-177 + smooth_l1 (beta < 1e-5: L1) of foreground anchor `a` of the tile -> loss; g = d loss / d delta
template <typename T>
__device__ __forceinline__ float rl_box_row(const RlTile& t, const float* __restrict__ gt_boxes, const RlParams& p, int a,
                                            float (&g)[5]) {
  const float* an = t.anchors + (long)(t.a0 + a) * 5;
  const float* gb = gt_boxes + ((long)t.n * p.R + t.col0 + a) * 5;
  const T* dr = (const T*)t.deltas + ((long)t.n * t.A + t.a0 + a) * 5;
  const double cx = an[0], cy = an[1], w = an[2], h = an[3], ang = an[4];
  const double tcx = gb[0], tcy = gb[1], tw = gb[2], th = gb[3], tang = gb[4];
  double da = fmod(tang - ang + 180.0, 360.0);  // torch's `%`: the result takes the divisor's sign
  if (da < 0.0) da += 360.0;
  da -= 180.0;
  const double tgt[5] = {(double)p.w[0] * (tcx - cx) / w, (double)p.w[1] * (tcy - cy) / h, (double)p.w[2] * log(tw / w),
                         (double)p.w[3] * log(th / h), da * ((double)p.w[4] * 3.141592653589793 / 180.0)};
  const double beta = p.beta;
  double loss = 0.0;
#pragma unroll
  for (int i = 0; i < 5; i++) {
    const double r = (double)to_f32(dr[i]) - tgt[i], n = fabs(r);
    const float sgn = r > 0.0 ? 1.f : (r < 0.0 ? -1.f : 0.f);
    if (p.beta < 1e-5f || !(n < beta)) {
      loss += p.beta < 1e-5f ? n : n - 0.5 * beta;
      g[i] = sgn;
    } else {
      loss += 0.5 * n * n / beta;
      g[i] = (float)(r / beta);
    }
  }
  return (float)loss;
}

template <typename T>
__global__ __launch_bounds__(RL_THREADS) void d2amd_rrpn_loss_forward_kernel(RlLevels P, RlParams p,
                                                                             const int8_t* __restrict__ gt_labels,
                                                                             const float* __restrict__ gt_boxes,
                                                                             RlPartial* __restrict__ partials) {
  __shared__ float s_red[RL_THREADS / 64][2];
  __shared__ int s_cnt[RL_THREADS / 64][2];
  const int tid = threadIdx.x;
  const RlTile t = rl_tile(P, blockIdx.x);
  const int code = rl_code(gt_labels, p, t, tid);
  float cls = 0.f, box = 0.f;
  if (code >= 0) cls = dl_focal<0>(to_f32(((const T*)t.logits)[(long)t.n * t.A + t.a0 + tid]), code, 0, p);
  if (code == 0) {
    float g[5];
    box = rl_box_row<T>(t, gt_boxes, p, tid, g);
  }
  const int fg = __popcll(__ballot(code == 0)), valid = __popcll(__ballot(code >= 0));
  cls = dl_wave_sum(cls);
  box = dl_wave_sum(box);
  if ((tid & 63) == 0) { s_red[tid >> 6][0] = cls; s_red[tid >> 6][1] = box; s_cnt[tid >> 6][0] = fg; s_cnt[tid >> 6][1] = valid; }
  __syncthreads();
  if (tid == 0) {
    RlPartial o;
    o.cls = ((s_red[0][0] + s_red[1][0]) + s_red[2][0]) + s_red[3][0];  // fixed order
    o.box = ((s_red[0][1] + s_red[1][1]) + s_red[2][1]) + s_red[3][1];
    o.fg = s_cnt[0][0] + s_cnt[1][0] + s_cnt[2][0] + s_cnt[3][0];
    o.valid = s_cnt[0][1] + s_cnt[1][1] + s_cnt[2][1] + s_cnt[3][1];
    partials[blockIdx.x] = o;
  }
}

__global__ __launch_bounds__(256) void d2amd_rrpn_loss_final_kernel(const RlPartial* __restrict__ partials, int tiles,
                                                                   float* __restrict__ loss_cls,
                                                                   float* __restrict__ loss_box,
                                                                   int64_t* __restrict__ stats) {
  const int tid = threadIdx.x;
  double c = 0., b = 0.;
  long fg = 0, valid = 0;
  for (int i = tid; i < tiles; i += 256) {
    const RlPartial v = partials[i];
    c += (double)v.cls; b += (double)v.box; fg += v.fg; valid += v.valid;
  }
  __shared__ double sc[256], sb[256];
  __shared__ long sf[256], sv[256];
  sc[tid] = c; sb[tid] = b; sf[tid] = fg; sv[tid] = valid;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {  // fixed tree: deterministic
    if (tid < s) { sc[tid] += sc[tid + s]; sb[tid] += sb[tid + s]; sf[tid] += sf[tid + s]; sv[tid] += sv[tid + s]; }
    __syncthreads();
  }
  if (tid == 0) {
    *loss_cls = (float)sc[0];
    *loss_box = (float)sb[0];
    stats[0] = sf[0];
    stats[1] = sv[0];
  }
}

template <typename T>
__global__ __launch_bounds__(RL_THREADS) void d2amd_rrpn_loss_backward_kernel(RlLevels P, RlParams p,
                                                                              const int8_t* __restrict__ gt_labels,
                                                                              const float* __restrict__ gt_boxes,
                                                                              const float* __restrict__ grad_cls,
                                                                              const float* __restrict__ grad_box) {
  __shared__ float s_g[RL_TILE * 5];
  const int tid = threadIdx.x;
  const RlTile t = rl_tile(P, blockIdx.x);
  const int code = rl_code(gt_labels, p, t, tid);
  const long e0 = (long)t.n * t.A + t.a0;
  if (tid < t.cnt) {
    float gx = 0.f;
    if (code >= 0) gx = dl_focal_grad<0>(to_f32(((const T*)t.logits)[e0 + tid]), code, 0, p, *grad_cls);
    ((T*)t.glogits)[e0 + tid] = from_f32<T>(gx);
  }
  float gd[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  if (code == 0) {
    rl_box_row<T>(t, gt_boxes, p, tid, gd);
    const float gb = *grad_box;
#pragma unroll
    for (int i = 0; i < 5; i++) gd[i] *= gb;
  }
#pragma unroll
  for (int i = 0; i < 5; i++) s_g[tid * 5 + i] = gd[i];
  __syncthreads();
  T* out = (T*)t.gdeltas + e0 * 5;
  for (int j = tid; j < t.cnt * 5; j += RL_THREADS) out[j] = from_f32<T>(s_g[j]);
}

}  // namespace d2amd

using namespace d2amd;

// level table + the argument checks the three entries share; -> number of tiles in *tiles
static int rl_layout(const char* op, int N, const int* level_anchors, int L, RlLevels& P, int* R, long* tiles) {
  D2_CHECK_ARG(N >= 0 && L >= 0 && L <= RL_MAX_LEVELS && (L == 0 || level_anchors),
               "%s: bad shape (N %d, %d levels [max %d])", op, N, L, RL_MAX_LEVELS);
  P = RlLevels{};
  P.L = L;
  long r = 0, t = 0;
  for (int l = 0; l < L; l++) {
    D2_CHECK_ARG(level_anchors[l] >= 0, "%s: level %d has a negative size", op, l);
    P.A[l] = level_anchors[l];
    P.aoff[l] = (int)r;
    P.tile_base[l] = (int)t;
    r += level_anchors[l];
    t += (long)N * ((level_anchors[l] + RL_TILE - 1) / RL_TILE);
    D2_CHECK_ARG(r < (1l << 31) && t < (1l << 31), "%s: too many anchors", op);
  }
  for (int l = L; l <= RL_MAX_LEVELS; l++) P.tile_base[l] = (int)t;
  *R = (int)r;
  *tiles = t;
  return D2AMD_OK;
}

static int rl_params(const char* op, int dtype, float beta, const float* weights, RlParams& p) {
  D2_CHECK_ARG(dtype == D2AMD_F32 || dtype == D2AMD_F16 || dtype == D2AMD_BF16, "%s: bad dtype code %d", op, dtype);
  D2_CHECK_ARG(beta >= 0.f, "%s: smooth_l1_beta %g < 0", op, beta);
  D2_CHECK_ARG(weights != nullptr, "%s: null weights", op);
  for (int i = 0; i < 5; i++) {
    D2_CHECK_ARG(weights[i] > 0.f, "%s: box weights must be positive", op);
    p.w[i] = weights[i];
  }
  p.alpha = -1.f; p.gamma = 0.f; p.beta = beta;
  return D2AMD_OK;
}

extern "C" size_t d2amd_rrpn_loss_workspace_bytes(int N, const int* level_anchors, int L) {
  RlLevels P; int R; long tiles;
  if (rl_layout("rrpn_loss_workspace_bytes", N, level_anchors, L, P, &R, &tiles)) return sizeof(RlPartial);
  return sizeof(RlPartial) * (size_t)(tiles > 0 ? tiles : 1);
}

extern "C" int d2amd_rrpn_loss_forward(const void* const* logits, const void* const* deltas, const float* const* anchors,
                                       const int8_t* gt_labels, const float* gt_boxes, int N, const int* level_anchors,
                                       int L, int dtype, float smooth_l1_beta, const float* weights, float* loss_cls_sum,
                                       float* loss_box_sum, int64_t* stats, void* workspace, size_t workspace_bytes,
                                       void* stream) {
  const char* op = "rrpn_loss_forward";
  RlLevels P; RlParams p{}; int R; long tiles;
  int rc = rl_layout(op, N, level_anchors, L, P, &R, &tiles);
  if (rc) return rc;
  rc = rl_params(op, dtype, smooth_l1_beta, weights, p);
  if (rc) return rc;
  p.N = N; p.R = R;
  if (tiles == 0) return D2AMD_OK;
  D2_CHECK_ARG(logits && deltas && anchors && gt_labels && gt_boxes, "%s: null pointer", op);
  D2_CHECK_ARG(loss_cls_sum && loss_box_sum && stats, "%s: null output", op);
  D2_CHECK_ARG(workspace && ((uintptr_t)workspace & 7) == 0 && workspace_bytes >= sizeof(RlPartial) * (size_t)tiles,
               "%s: workspace missing, not 8-byte aligned or too small (%zu bytes, %zu needed)", op, workspace_bytes,
               sizeof(RlPartial) * (size_t)tiles);
  for (int l = 0; l < L; l++) {
    if (level_anchors[l] == 0) continue;
    D2_CHECK_ARG(logits[l] && deltas[l] && anchors[l], "%s: null level %d", op, l);
    P.logits[l] = logits[l]; P.deltas[l] = deltas[l]; P.anchors[l] = anchors[l];
  }
  hipStream_t s = (hipStream_t)stream;
  RlPartial* partials = (RlPartial*)workspace;
  rc = D2_DISPATCH_DTYPE(dtype, [&]() -> int {
    hipLaunchKernelGGL((d2amd_rrpn_loss_forward_kernel<scalar_t>), dim3((unsigned)tiles), dim3(RL_THREADS), 0, s, P, p,
                       gt_labels, gt_boxes, partials);
    D2_LAUNCH_OK();
    return D2AMD_OK;
  });
  if (rc) return rc;
  hipLaunchKernelGGL(d2amd_rrpn_loss_final_kernel, dim3(1), dim3(256), 0, s, partials, (int)tiles, loss_cls_sum,
                     loss_box_sum, stats);
  D2_LAUNCH_OK();
  return D2AMD_OK;
}

extern "C" int d2amd_rrpn_loss_backward(const void* const* logits, const void* const* deltas, const float* const* anchors,
                                        const int8_t* gt_labels, const float* gt_boxes, const float* grad_cls,
                                        const float* grad_box, int N, const int* level_anchors, int L, int dtype,
                                        float smooth_l1_beta, const float* weights, void* const* grad_logits,
                                        void* const* grad_deltas, void* stream) {
  const char* op = "rrpn_loss_backward";
  RlLevels P; RlParams p{}; int R; long tiles;
  int rc = rl_layout(op, N, level_anchors, L, P, &R, &tiles);
  if (rc) return rc;
  rc = rl_params(op, dtype, smooth_l1_beta, weights, p);
  if (rc) return rc;
  p.N = N; p.R = R;
  if (tiles == 0) return D2AMD_OK;
  D2_CHECK_ARG(logits && deltas && anchors && gt_labels && gt_boxes && grad_cls && grad_box && grad_logits && grad_deltas,
               "%s: null pointer", op);
  for (int l = 0; l < L; l++) {
    if (level_anchors[l] == 0) continue;
    D2_CHECK_ARG(logits[l] && deltas[l] && anchors[l] && grad_logits[l] && grad_deltas[l], "%s: null level %d", op, l);
    P.logits[l] = logits[l]; P.deltas[l] = deltas[l]; P.anchors[l] = anchors[l];
    P.glogits[l] = grad_logits[l]; P.gdeltas[l] = grad_deltas[l];
  }
  hipStream_t s = (hipStream_t)stream;
  return D2_DISPATCH_DTYPE(dtype, [&]() -> int {
    hipLaunchKernelGGL((d2amd_rrpn_loss_backward_kernel<scalar_t>), dim3((unsigned)tiles), dim3(RL_THREADS), 0, s, P, p,
                       gt_labels, gt_boxes, grad_cls, grad_box);
    D2_LAUNCH_OK();
    return D2AMD_OK;
  });
}
