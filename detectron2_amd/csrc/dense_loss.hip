// Training losses of the dense-anchor detectors, fused: classification (sigmoid focal / BCE) + box regression of ALL
// images and levels in one forward and one backward launch.
//   replaces  detectron2/modeling/meta_arch/retinanet.py:160-210 (RetinaNet.losses: cat of the per-level logits, a boolean
//             index of the N x R x K result, a one-hot of the same size, sigmoid_focal_loss_jit, `.item()` on the number
//             of foreground anchors, and autograd back through every copy),
//             detectron2/modeling/proposal_generator/rpn.py:366-429 (RPN.losses: the same with K = 1 and plain BCE, two
//             `.item()`s) and
//             detectron2/modeling/box_regression.py:310-369 (_dense_box_regression_loss: get_deltas / apply_deltas over all
//             N x R anchors, then the foreground index; smooth_l1 and giou here).
// Here:
//   * a WORKGROUP (256 threads) OWNS A TILE of DL_TILE = 256 consecutive anchors of one (image, level); the level table
//     (per-level pointers + A_l + prefix of tiles) is a by-value kernel argument, nothing is concatenated.
//       1. the tile's labels go to LDS once as a code: -1 ignore, K background, c < K foreground of class c (the
//          objectness mode maps 1 -> class 0, 0 -> K = 1); ballots count the foreground and the valid rows;
//       2. the tile's cnt * K contiguous logits are streamed with 16-byte loads: up to 15 bytes of head to the next
//          16-byte boundary and the tail behind the last whole vector go through element accesses (an odd A_l * K puts
//          image 1's base anywhere).  An element's (anchor, class) is one division per vector, then counted up; the
//          target is `LDS label == class`.  A tile without a valid row loads no logit in the forward;
//       3. thread i then does anchor i's box term if it is foreground (a few per tile): anchor, delta row, matched box.
//   * focal term on z = (t ? -x : x), for which 1 - p_t = sigmoid(z) and ce = softplus(z):
//       e = exp(-|x|), l = log(1 + e), ce = max(z, 0) + l, q = sigmoid(z) = (z >= 0 ? 1 : e) / (1 + e),
//       loss = w ce q^g,   dloss/dz = w q^g (q + g ce (1 - q)),   w = alpha_t or 1 (alpha < 0)
//     q^g is 1 (g = 0: plain BCE, no pow anywhere), q * q (g = 2) or exp(g log q) with log q = -(max(-z, 0) + l): every
//     logarithm goes through the softplus form and is finite for any finite x (q = 0 gives exp(-large) = 0, never
//     0 * inf).  The backward recomputes this from x: nothing per element is saved by the forward.
//     exp / log are the hardware's exp2 / log2 (v_exp_f32, v_log_f32, 1 ulp): the arguments are <= 0 and in [1, 2].
//   * reductions: butterfly inside a wave, four waves added in order, one (cls, box, #fg, #valid) record per tile in the
//     workspace; a one-workgroup kernel adds the records in fp64 in a fixed order.  No float atomics: bit-identical runs.
//   * backward: same tiling, reads the two upstream gradients from device scalars and writes EVERY element of every
//     level's logit and delta gradient once, zeros included (ignored / background rows; a tile without a valid row is
//     written without reading its logits).
// Roofline (RetinaNet, 2 x 800 x 1344, K = 80, bf16: 32.3 M logits): forward reads 64.5 MB, backward reads 64.5 MB and
// writes 64.5 MB; three quarter-rate transcendentals per element put the VALU time in the same range.
#include "common.h"
#include "loss_common.h"

namespace d2amd {

constexpr int DL_TILE = 256;     // anchors per workgroup
constexpr int DL_THREADS = 256;  // == DL_TILE: thread i owns anchor i of the tile in the box term
constexpr int DL_MAX_LEVELS = D2AMD_RPN_MAX_LEVELS;

struct DlLevels {
  const void* logits[DL_MAX_LEVELS];   // [N, A_l, K]
  const void* deltas[DL_MAX_LEVELS];   // [N, A_l, 4]
  const float* anchors[DL_MAX_LEVELS]; // [A_l, 4]
  void* glogits[DL_MAX_LEVELS];        // backward only
  void* gdeltas[DL_MAX_LEVELS];
  int A[DL_MAX_LEVELS];
  int aoff[DL_MAX_LEVELS];             // prefix of A_l: the level's first column of gt_labels / gt_boxes
  int tile_base[DL_MAX_LEVELS + 1];    // prefix of N * cdiv(A_l, DL_TILE); entries behind L repeat the total
  int L;
};

struct DlParams {
  int N, K, R;
  int objectness;   // label mode
  float alpha, gamma;
  int giou;         // box term: 0 smooth_l1, 1 giou
  float beta, wx, wy, ww, wh, scale_clamp;
};

struct DlPartial { float cls, box; int fg, valid; };  // one per tile

// ---- the tile of a workgroup -------------------------------------------------------------------------------------
struct DlTile {
  const void* logits; const void* deltas; const float* anchors; void* glogits; void* gdeltas;
  int A, col0, n, a0, cnt;  // col0: column of anchor a0 in gt_labels / gt_boxes
};

__device__ __forceinline__ DlTile dl_tile(const DlLevels& P, int b) {
  int l = 0;
#pragma unroll
  for (int q = 1; q < DL_MAX_LEVELS; q++)
    if (q < P.L && b >= P.tile_base[q]) l = q;
  DlTile t{};
  int base = 0, aoff = 0;
#pragma unroll
  for (int q = 0; q < DL_MAX_LEVELS; q++)  // (selects: no runtime index into the by-value argument)
    if (q == l) {
      t.logits = P.logits[q]; t.deltas = P.deltas[q]; t.anchors = P.anchors[q];
      t.glogits = P.glogits[q]; t.gdeltas = P.gdeltas[q];
      t.A = P.A[q]; aoff = P.aoff[q]; base = P.tile_base[q];
    }
  const int per_image = (t.A + DL_TILE - 1) / DL_TILE;
  const int r = b - base;
  t.n = r / per_image;
  t.a0 = (r - t.n * per_image) * DL_TILE;
  t.cnt = min(DL_TILE, t.A - t.a0);
  t.col0 = aoff + t.a0;
  return t;
}

// labels of the tile -> LDS codes; -> (#foreground, #valid) of the tile, the same in every thread.  s_lab has DL_TILE + 1
// entries (the streaming loop may step one anchor past the tile before it stops).
__device__ __forceinline__ int2 dl_stage_labels(const int64_t* __restrict__ gt_labels, const DlParams& p,
                                                const DlTile& t, int* s_lab, int* s_cnt) {
  const int tid = threadIdx.x;
  int code = -1;
  if (tid < t.cnt) {
    const int64_t v = gt_labels[(long)t.n * p.R + t.col0 + tid];
    if (p.objectness) code = v == 1 ? 0 : (v == 0 ? 1 : -1);  // K == 1
    else code = v < 0 ? -1 : (v >= p.K ? p.K : (int)v);
  }
  s_lab[tid] = code;
  if (tid == 0) { s_lab[DL_TILE] = -1; s_cnt[0] = 0; s_cnt[1] = 0; }
  __syncthreads();
  const int fg = __popcll(__ballot(code >= 0 && code < p.K)), valid = __popcll(__ballot(code >= 0));
  if ((tid & 63) == 0) { atomicAdd(&s_cnt[0], fg); atomicAdd(&s_cnt[1], valid); }  // integers: order-independent
  __syncthreads();
  return make_int2(s_cnt[0], s_cnt[1]);
}

// anchor `a` of the tile (foreground) -> its box loss and delta gradient
template <typename T>
__device__ __forceinline__ float dl_box_row(const DlTile& t, const float* __restrict__ gt_boxes, const DlParams& p, int a,
                                            float (&g)[4]) {
  const float* an = t.anchors + (long)(t.a0 + a) * 4;
  const float* gb = gt_boxes + ((long)t.n * p.R + t.col0 + a) * 4;
  const T* dr = (const T*)t.deltas + ((long)t.n * t.A + t.a0 + a) * 4;
  const float av[4] = {an[0], an[1], an[2], an[3]}, gv[4] = {gb[0], gb[1], gb[2], gb[3]};
  const float dv[4] = {to_f32(dr[0]), to_f32(dr[1]), to_f32(dr[2]), to_f32(dr[3])};
  return dl_box_term(av, gv, dv, p, g);
}

// ---- forward ---------------------------------------------------------------------------------------------------
template <typename T, int GM>
__global__ __launch_bounds__(DL_THREADS) void d2amd_dense_loss_forward_kernel(DlLevels P, DlParams p,
                                                                              const int64_t* __restrict__ gt_labels,
                                                                              const float* __restrict__ gt_boxes,
                                                                              int vec, DlPartial* __restrict__ partials) {
  __shared__ int s_lab[DL_TILE + 1];
  __shared__ int s_cnt[2];
  __shared__ float s_red[DL_THREADS / 64][2];
  const int tid = threadIdx.x;
  const DlTile t = dl_tile(P, blockIdx.x);
  const int2 counts = dl_stage_labels(gt_labels, p, t, s_lab, s_cnt);
  float cls = 0.f, box = 0.f;
  if (counts.y > 0) {  // (the same in every thread)
    constexpr int V = dl_vec<T>::N;
    const int K = p.K, count = t.cnt * K;
    const T* x = (const T*)t.logits + ((long)t.n * t.A + t.a0) * K;
    const int head = dl_head(x, count, vec != 0);
    const int nvec = (count - head) / V, tail0 = head + nvec * V;
    for (int j = tid; j < head; j += DL_THREADS) {
      const int a = j / K;
      cls += dl_focal<GM>(to_f32(x[j]), s_lab[a], j - a * K, p);
    }
    for (int i = tid; i < nvec; i += DL_THREADS) {
      float e[V];
      const int j0 = head + i * V;
      dl_load16(x + j0, e);
      int a = j0 / K, c = j0 - a * K;
#pragma unroll
      for (int q = 0; q < V; q++) {
        cls += dl_focal<GM>(e[q], s_lab[a], c, p);
        const bool wrap = ++c == K;
        c = wrap ? 0 : c;
        a += wrap;
      }
    }
    {
      const int j = tail0 + tid;
      if (j < count) {
        const int a = j / K;
        cls += dl_focal<GM>(to_f32(x[j]), s_lab[a], j - a * K, p);
      }
    }
    const int code = s_lab[tid];
    if (code >= 0 && code < K) {
      float g[4];
      box = dl_box_row<T>(t, gt_boxes, p, tid, g);
    }
  }
  cls = dl_wave_sum(cls);
  box = dl_wave_sum(box);
  if ((tid & 63) == 0) { s_red[tid >> 6][0] = cls; s_red[tid >> 6][1] = box; }
  __syncthreads();
  if (tid == 0) {
    DlPartial o;
    o.cls = ((s_red[0][0] + s_red[1][0]) + s_red[2][0]) + s_red[3][0];  // fixed order
    o.box = ((s_red[0][1] + s_red[1][1]) + s_red[2][1]) + s_red[3][1];
    o.fg = counts.x; o.valid = counts.y;
    partials[blockIdx.x] = o;
  }
}

__global__ __launch_bounds__(256) void d2amd_dense_loss_final_kernel(const DlPartial* __restrict__ partials, int tiles,
                                                                    float* __restrict__ loss_cls,
                                                                    float* __restrict__ loss_box,
                                                                    int64_t* __restrict__ stats) {
  const int tid = threadIdx.x;
  double c = 0., b = 0.;
  long fg = 0, valid = 0;
  for (int i = tid; i < tiles; i += 256) {
    const DlPartial v = partials[i];
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

// ---- backward --------------------------------------------------------------------------------------------------
template <typename T, int GM>
__global__ __launch_bounds__(DL_THREADS) void d2amd_dense_loss_backward_kernel(DlLevels P, DlParams p,
                                                                               const int64_t* __restrict__ gt_labels,
                                                                               const float* __restrict__ gt_boxes,
                                                                               const float* __restrict__ grad_cls,
                                                                               const float* __restrict__ grad_box,
                                                                               int vec) {
  __shared__ int s_lab[DL_TILE + 1];
  __shared__ int s_cnt[2];
  const int tid = threadIdx.x;
  const DlTile t = dl_tile(P, blockIdx.x);
  const int2 counts = dl_stage_labels(gt_labels, p, t, s_lab, s_cnt);
  constexpr int V = dl_vec<T>::N;
  const int K = p.K, count = t.cnt * K;
  const long e0 = ((long)t.n * t.A + t.a0) * K;
  const T* x = (const T*)t.logits + e0;
  T* gx = (T*)t.glogits + e0;
  const int head = dl_head(gx, count, vec != 0);  // (vec: logits and gradient share their offset inside 16 bytes)
  const int nvec = (count - head) / V, tail0 = head + nvec * V;
  if (counts.y == 0) {  // nothing valid: zeros, the logits are not read
    float z[V];
#pragma unroll
    for (int q = 0; q < V; q++) z[q] = 0.f;
    for (int j = tid; j < head; j += DL_THREADS) gx[j] = from_f32<T>(0.f);
    for (int i = tid; i < nvec; i += DL_THREADS) dl_store16(gx + head + i * V, z);
    if (tail0 + tid < count) gx[tail0 + tid] = from_f32<T>(0.f);
  } else {
    const float g = *grad_cls;
    for (int j = tid; j < head; j += DL_THREADS) {
      const int a = j / K;
      gx[j] = from_f32<T>(dl_focal_grad<GM>(to_f32(x[j]), s_lab[a], j - a * K, p, g));
    }
    for (int i = tid; i < nvec; i += DL_THREADS) {
      float e[V];
      const int j0 = head + i * V;
      dl_load16(x + j0, e);
      int a = j0 / K, c = j0 - a * K;
#pragma unroll
      for (int q = 0; q < V; q++) {
        e[q] = dl_focal_grad<GM>(e[q], s_lab[a], c, p, g);
        const bool wrap = ++c == K;
        c = wrap ? 0 : c;
        a += wrap;
      }
      dl_store16(gx + j0, e);
    }
    {
      const int j = tail0 + tid;
      if (j < count) {
        const int a = j / K;
        gx[j] = from_f32<T>(dl_focal_grad<GM>(to_f32(x[j]), s_lab[a], j - a * K, p, g));
      }
    }
  }
  // the delta gradient: one row of four per thread (rows are 4 * sizeof(T)-aligned: checked on the host)
  if (tid < t.cnt) {
    float gd[4] = {0.f, 0.f, 0.f, 0.f};
    const int code = s_lab[tid];
    if (code >= 0 && code < K) {
      dl_box_row<T>(t, gt_boxes, p, tid, gd);
      const float gb = *grad_box;
#pragma unroll
      for (int i = 0; i < 4; i++) gd[i] *= gb;
    }
    vec4<T> o;
    pack4(gd, o);
    *reinterpret_cast<vec4<T>*>((T*)t.gdeltas + ((long)t.n * t.A + t.a0 + tid) * 4) = o;
  }
}

}  // namespace d2amd

using namespace d2amd;

// level table + argument checks shared by the three entries; -> number of tiles in *tiles
static int dl_layout(const char* op, int N, const int* level_anchors, int L, int K, DlLevels& P, int* R, long* tiles) {
  D2_CHECK_ARG(N >= 0 && L >= 0 && L <= DL_MAX_LEVELS && (L == 0 || level_anchors) && K >= 1 && K < (1 << 22),
               "%s: bad shape (N %d, %d levels [max %d], K %d)", op, N, L, DL_MAX_LEVELS, K);
  P = DlLevels{};
  P.L = L;
  long r = 0, t = 0;
  for (int l = 0; l < L; l++) {
    D2_CHECK_ARG(level_anchors[l] >= 0 && (long)level_anchors[l] * K < (1l << 31), "%s: level %d too large", op, l);
    P.A[l] = level_anchors[l];
    P.aoff[l] = (int)r;
    P.tile_base[l] = (int)t;
    r += level_anchors[l];
    t += (long)N * ((level_anchors[l] + DL_TILE - 1) / DL_TILE);
    D2_CHECK_ARG(r < (1l << 31) && t < (1l << 31), "%s: too many anchors", op);
  }
  for (int l = L; l <= DL_MAX_LEVELS; l++) P.tile_base[l] = (int)t;
  *R = (int)r;
  *tiles = t;
  return D2AMD_OK;
}

static int dl_params(const char* op, int K, int label_mode, float alpha, float gamma, int box_loss, float beta,
                     const float* weights, float scale_clamp, DlParams& p) {
  if (label_mode != D2AMD_DENSE_LABELS_CLASS && label_mode != D2AMD_DENSE_LABELS_OBJECTNESS) {
    set_error("%s: label mode %d (class 0, objectness 1)", op, label_mode);
    return D2AMD_EUNSUPPORTED;
  }
  if (box_loss != D2AMD_BOX_LOSS_SMOOTH_L1 && box_loss != D2AMD_BOX_LOSS_GIOU) {
    set_error("%s: box loss %d (smooth_l1 0, giou 1; diou / ciou are not implemented)", op, box_loss);
    return D2AMD_EUNSUPPORTED;
  }
  D2_CHECK_ARG(label_mode != D2AMD_DENSE_LABELS_OBJECTNESS || K == 1, "%s: objectness labels need K == 1, got %d", op, K);
  D2_CHECK_ARG(gamma >= 0.f && gamma == gamma && alpha <= 1.f && beta >= 0.f, "%s: gamma %g < 0, alpha %g > 1 or beta %g < 0",
               op, gamma, alpha, beta);
  D2_CHECK_ARG(weights && weights[0] > 0.f && weights[1] > 0.f && weights[2] > 0.f && weights[3] > 0.f,
               "%s: box weights must be positive", op);
  p.K = K; p.objectness = label_mode == D2AMD_DENSE_LABELS_OBJECTNESS;
  p.alpha = alpha; p.gamma = gamma; p.giou = box_loss == D2AMD_BOX_LOSS_GIOU; p.beta = beta;
  p.wx = weights[0]; p.wy = weights[1]; p.ww = weights[2]; p.wh = weights[3]; p.scale_clamp = scale_clamp;
  return D2AMD_OK;
}

// the three gamma variants of a kernel template for scalar_t
#define DL_LAUNCH(kernel, gamma, grid, s, ...)                                                                         \
  do {                                                                                                                 \
    if ((gamma) == 0.f)                                                                                                \
      hipLaunchKernelGGL((kernel<scalar_t, 0>), grid, dim3(DL_THREADS), 0, s, __VA_ARGS__);                            \
    else if ((gamma) == 2.f)                                                                                           \
      hipLaunchKernelGGL((kernel<scalar_t, 2>), grid, dim3(DL_THREADS), 0, s, __VA_ARGS__);                            \
    else                                                                                                               \
      hipLaunchKernelGGL((kernel<scalar_t, 1>), grid, dim3(DL_THREADS), 0, s, __VA_ARGS__);                            \
  } while (0)

extern "C" size_t d2amd_dense_loss_workspace_bytes(int N, const int* level_anchors, int L) {
  DlLevels P; int R; long tiles;
  if (dl_layout("dense_loss_workspace_bytes", N, level_anchors, L, 1, P, &R, &tiles)) return sizeof(DlPartial);
  return sizeof(DlPartial) * (size_t)(tiles > 0 ? tiles : 1);
}

extern "C" int d2amd_dense_loss_forward(const void* const* logits, const void* const* deltas, const float* const* anchors,
                                        const int64_t* gt_labels, const float* gt_boxes, int N, const int* level_anchors,
                                        int L, int K, int dtype, int label_mode, float alpha, float gamma, int box_loss,
                                        float smooth_l1_beta, const float* weights, float scale_clamp,
                                        float* loss_cls_sum, float* loss_box_sum, int64_t* stats, void* workspace,
                                        size_t workspace_bytes, void* stream) {
  const char* op = "dense_loss_forward";
  DlLevels P; DlParams p{}; int R; long tiles;
  int rc = dl_layout(op, N, level_anchors, L, K, P, &R, &tiles);
  if (rc) return rc;
  rc = dl_params(op, K, label_mode, alpha, gamma, box_loss, smooth_l1_beta, weights, scale_clamp, p);
  if (rc) return rc;
  p.N = N; p.R = R;
  D2_CHECK_ARG(loss_cls_sum && loss_box_sum && stats, "%s: null output", op);
  D2_CHECK_ARG(workspace && ((uintptr_t)workspace & 7) == 0 && workspace_bytes >= sizeof(DlPartial) * (size_t)(tiles > 0 ? tiles : 1),
               "%s: workspace missing, not 8-byte aligned or too small (%zu bytes, %zu needed)", op, workspace_bytes,
               sizeof(DlPartial) * (size_t)(tiles > 0 ? tiles : 1));
  hipStream_t s = (hipStream_t)stream;
  DlPartial* partials = (DlPartial*)workspace;
  if (tiles > 0) {
    D2_CHECK_ARG(logits && deltas && anchors && gt_labels && gt_boxes, "%s: null pointer", op);
    bool vec = true;
    for (int l = 0; l < L; l++) {
      if (level_anchors[l] == 0) continue;
      D2_CHECK_ARG(logits[l] && deltas[l] && anchors[l], "%s: null level %d", op, l);
      P.logits[l] = logits[l]; P.deltas[l] = deltas[l]; P.anchors[l] = anchors[l];
      vec = vec && ((uintptr_t)logits[l] % dtype_size(dtype)) == 0;
    }
    rc = D2_DISPATCH_DTYPE(dtype, [&]() -> int {
      DL_LAUNCH(d2amd_dense_loss_forward_kernel, gamma, dim3((unsigned)tiles), s, P, p, gt_labels, gt_boxes, (int)vec,
                partials);
      D2_LAUNCH_OK();
      return D2AMD_OK;
    });
    if (rc) return rc;
  } else if (dtype != D2AMD_F32 && dtype != D2AMD_F16 && dtype != D2AMD_BF16) {
    set_error("unsupported dtype %d", dtype);
    return D2AMD_EUNSUPPORTED;
  }
  hipLaunchKernelGGL(d2amd_dense_loss_final_kernel, dim3(1), dim3(256), 0, s, partials, (int)tiles, loss_cls_sum,
                     loss_box_sum, stats);
  D2_LAUNCH_OK();
  return D2AMD_OK;
}

extern "C" int d2amd_dense_loss_backward(const void* const* logits, const void* const* deltas,
                                         const float* const* anchors, const int64_t* gt_labels, const float* gt_boxes,
                                         const float* grad_cls, const float* grad_box, int N, const int* level_anchors,
                                         int L, int K, int dtype, int label_mode, float alpha, float gamma, int box_loss,
                                         float smooth_l1_beta, const float* weights, float scale_clamp,
                                         void* const* grad_logits, void* const* grad_deltas, void* stream) {
  const char* op = "dense_loss_backward";
  DlLevels P; DlParams p{}; int R; long tiles;
  int rc = dl_layout(op, N, level_anchors, L, K, P, &R, &tiles);
  if (rc) return rc;
  rc = dl_params(op, K, label_mode, alpha, gamma, box_loss, smooth_l1_beta, weights, scale_clamp, p);
  if (rc) return rc;
  p.N = N; p.R = R;
  if (tiles == 0) {
    if (dtype != D2AMD_F32 && dtype != D2AMD_F16 && dtype != D2AMD_BF16) {
      set_error("unsupported dtype %d", dtype);
      return D2AMD_EUNSUPPORTED;
    }
    return D2AMD_OK;
  }
  D2_CHECK_ARG(logits && deltas && anchors && gt_labels && gt_boxes && grad_cls && grad_box && grad_logits && grad_deltas,
               "%s: null pointer", op);
  const size_t es = dtype_size(dtype);
  bool vec = true;
  for (int l = 0; l < L; l++) {
    if (level_anchors[l] == 0) continue;
    D2_CHECK_ARG(logits[l] && deltas[l] && anchors[l] && grad_logits[l] && grad_deltas[l], "%s: null level %d", op, l);
    D2_CHECK_ARG(((uintptr_t)grad_deltas[l] & (4 * es - 1)) == 0, "%s: grad_deltas[%d] is not aligned to a row of four", op, l);
    P.logits[l] = logits[l]; P.deltas[l] = deltas[l]; P.anchors[l] = anchors[l];
    P.glogits[l] = grad_logits[l]; P.gdeltas[l] = grad_deltas[l];
    // 16-byte vectors need the logits and their gradient at the same offset inside 16 bytes, on an element boundary
    vec = vec && (((uintptr_t)logits[l] ^ (uintptr_t)grad_logits[l]) & 15) == 0 && ((uintptr_t)logits[l] % es) == 0;
  }
  hipStream_t s = (hipStream_t)stream;
  return D2_DISPATCH_DTYPE(dtype, [&]() -> int {
    DL_LAUNCH(d2amd_dense_loss_backward_kernel, gamma, dim3((unsigned)tiles), s, P, p, gt_labels, gt_boxes, grad_cls,
              grad_box, (int)vec);
    D2_LAUNCH_OK();
    return D2AMD_OK;
  });
}
