// Training loss of the box head, fused: classification (softmax cross-entropy or sigmoid BCE with a class mask) + box
// regression of all sampled rows in one forward and one backward launch set.
//   replaces  detectron2/modeling/roi_heads/fast_rcnn.py:307-352 (FastRCNNOutputLayers.losses), :88-115
//             (_log_classification_stats: an argmax and four nonzero() host reads), :386-422 (sigmoid_cross_entropy_loss:
//             an R x (K+1) one-hot) and :424-463 (box_reg_loss: a fifth nonzero(), a two-level gather of the class's four
//             deltas, get_deltas / apply_deltas, and autograd back through every copy).
// Rows: class in [0, K) foreground, K background, anything else (the sampler's -1) padding: no loss, no statistic, zero
// gradient, not in the normaliser.  Both terms are divided by the number of rows that count, counted here.
// Here:
//   * a WORKGROUP (4 waves) OWNS `rpw` CONSECUTIVE ROWS (rpw = 4 ... 32, chosen on the host: the largest power of two
//     that still gives 256 workgroups, so R = 1024 fills the machine with one row per wave, and whose rows fit 60 KB of
//     LDS, so K = 1203 takes 16 bf16 / 8 fp32 rows; fewer than 4 only when K alone asks for it).  Rows are K + 1 elements
//     long, so a row's base is aligned to nothing; but the workgroup's rows are ONE contiguous span:
//       1. the classes of the rows go to LDS as codes (-1 / class);
//       2. the span is copied to LDS with 16-byte loads, kept in the I/O dtype and at the span's own offset inside 16 bytes
//          so that LDS and memory vectors coincide; up to 15 bytes of head and the tail go by element.  A vector that
//          lies in padding rows only is not loaded, and nothing of a padding row is ever used;
//       3. wave w reduces rows w, w + 4, ... from LDS, lanes striding the row ONCE: running maximum, its index (lowest on
//          ties: torch.argmax's CPU rule), and the sum of exp(x - max) rescaled when the maximum moves; the 64 partial
//          (max, index, sum) triples are merged by a butterfly.  loss = log(sum) - (x[target] - max).  The sigmoid mode
//          sums class_weight[c] * (max(x, 0) - x t + log(1 + exp(-|x|))) over the first K columns instead;
//       4. thread i does the box term of row i if it is foreground (dl_box_term of loss_common.h, the arithmetic the
//          dense-anchor losses use, here in fp64: a handful of rows per workgroup) on the row's own four deltas; its
//          ground-truth box is gt_boxes[r] or, in the sampler's form, table[offset[r / S] + gt_index[r]] (the index is
//          clamped to the table).
//   * exp / log are the hardware's exp2 / log2 (v_exp_f32, v_log_f32, 1 ulp) on arguments <= 0 and in [1, K + 1]: finite
//     for any finite logit.  (max, sum) of each row are kept apart in the workspace -- max + log(sum) in one fp32 would
//     cost an ulp of |max| -- and the backward's softmax is exp(x - max) / sum.
//   * reductions: thread 0 adds the workgroup's rows in order into one (cls, box, 5 counts) record; a one-workgroup
//     kernel adds the records in fp64 in a fixed order, divides by the row count and leaves that count for the backward.
//     No float atomics: two runs are bit-identical.
//   * backward: same tiling.  The span goes to LDS, each wave overwrites its rows IN LDS with the gradient (zeros for
//     padding rows, whose logits it does not read), and the span leaves with 16-byte stores: every element of
//     grad_scores is written once.  grad_deltas (R x 4K: the larger tensor, all zeros but four entries per foreground
//     row) is streamed with 16-byte stores straight from registers, the four entries merged from LDS.
// There is no contraction in this loss, so no MFMA: it is one read (forward), one read and two writes (backward) of
// memory with three transcendentals per logit; DESIGN.md 3.14 has the bytes and the measured times.
#include "common.h"
#include "loss_common.h"

namespace d2amd {

constexpr int BL_THREADS = 256;
constexpr int BL_WAVES = BL_THREADS / 64;
constexpr int BL_MAX_ROWS = 32;                 // rows of a workgroup
constexpr size_t BL_LDS_BYTES = 60 * 1024;      // the staged span (dynamic LDS)
constexpr size_t BL_HEADER_BYTES = 16;          // workspace: int64 row count | BlRow[R] | BlPartial[R]

struct BlParams {
  int R, K, C, D;   // C = K + 1 columns of scores, D = 4 or 4K columns of deltas
  int rpw;          // rows per workgroup
  int S, N, G;      // sampler form: rows per image, images, rows of the ground-truth table
  int giou;
  float beta, wx, wy, ww, wh, scale_clamp;
};

struct BlRow { float m, s; };                              // softmax: row maximum, sum of exp(x - m)
struct BlPartial { float cls, box; int n[5]; int pad; };   // one per workgroup

__device__ __forceinline__ float bl_shfl(float v, int o) { return __shfl_xor(v, o, 64); }

// classes of the workgroup's rows -> LDS codes (-1 padding, else the class); entries up to BL_MAX_ROWS are defined
__device__ __forceinline__ void bl_stage_codes(const int64_t* __restrict__ gt_classes, const BlParams& p, int r0, int nrows,
                                               int* s_code) {
  const int tid = threadIdx.x;
  if (tid <= BL_MAX_ROWS) {
    int code = -1;
    if (tid < nrows) {
      const int64_t v = gt_classes[r0 + tid];
      code = v >= 0 && v <= p.K ? (int)v : -1;
    }
    s_code[tid] = code;
  }
}

// the span x[0 .. count) -> s_x[0 .. count), both at the same offset inside 16 bytes when `vec`
template <typename T>
__device__ __forceinline__ void bl_stage_in(const T* __restrict__ x, int count, bool vec, int C, const int* s_code, T* s_x) {
  constexpr int V = dl_vec<T>::N;
  const int tid = threadIdx.x;
  const int head = dl_head(x, count, vec);
  const int nvec = (count - head) / V, tail0 = head + nvec * V;
  for (int j = tid; j < head; j += BL_THREADS)
    if (s_code[j / C] >= 0) s_x[j] = x[j];
  for (int i = tid; i < nvec; i += BL_THREADS) {
    const int j0 = head + i * V;
    const int a1 = (j0 + V - 1) / C;  // < rows: j0 + V <= count
    bool need = false;
    for (int a = j0 / C; a <= a1; a++) need = need || s_code[a] >= 0;
    if (need) *reinterpret_cast<uint4*>(s_x + j0) = *reinterpret_cast<const uint4*>(x + j0);
  }
  for (int j = tail0 + tid; j < count; j += BL_THREADS)
    if (s_code[j / C] >= 0) s_x[j] = x[j];
}

template <typename T>
__device__ __forceinline__ void bl_stage_out(const T* s_x, int count, bool vec, T* __restrict__ gx) {
  constexpr int V = dl_vec<T>::N;
  const int tid = threadIdx.x;
  const int head = dl_head(gx, count, vec);
  const int nvec = (count - head) / V, tail0 = head + nvec * V;
  for (int j = tid; j < head; j += BL_THREADS) gx[j] = s_x[j];
  for (int i = tid; i < nvec; i += BL_THREADS) {
    const int j0 = head + i * V;
    *reinterpret_cast<uint4*>(gx + j0) = *reinterpret_cast<const uint4*>(s_x + j0);
  }
  for (int j = tail0 + tid; j < count; j += BL_THREADS) gx[j] = s_x[j];
}

// box term of foreground row r (class `code`): -> loss, g = d loss / d (the row's four deltas)
template <typename T>
__device__ __forceinline__ float bl_box_row(const BlParams& p, int r, int code, const T* __restrict__ deltas,
                                            const float* __restrict__ boxes, const float* __restrict__ gt_boxes,
                                            const int64_t* __restrict__ gt_index, const int64_t* __restrict__ gt_offsets,
                                            float (&g)[4]) {
  long gi = r;
  if (gt_index != nullptr) {
    gi = gt_offsets[min(r / p.S, p.N - 1)] + gt_index[r];
    gi = gi < 0 ? 0 : (gi >= p.G ? p.G - 1 : gi);
  }
  const float* pb = boxes + (long)r * 4;
  const float* gb = gt_boxes + gi * 4;
  const T* dr = deltas + (long)r * p.D + (p.D == 4 ? 0 : 4 * code);
  const float av[4] = {pb[0], pb[1], pb[2], pb[3]}, gv[4] = {gb[0], gb[1], gb[2], gb[3]};
  const float dv[4] = {to_f32(dr[0]), to_f32(dr[1]), to_f32(dr[2]), to_f32(dr[3])};
  return dl_box_term<double>(av, gv, dv, p, g);  // (fp64: see loss_common.h)
}

// ---- forward ---------------------------------------------------------------------------------------------------
template <typename T, bool SIG>
__global__ __launch_bounds__(BL_THREADS) void d2amd_box_loss_forward_kernel(
    BlParams p, const T* __restrict__ scores, const T* __restrict__ deltas, const int64_t* __restrict__ gt_classes,
    const float* __restrict__ boxes, const float* __restrict__ gt_boxes, const int64_t* __restrict__ gt_index,
    const int64_t* __restrict__ gt_offsets, const float* __restrict__ class_weight, int vec, BlRow* __restrict__ rows_out,
    BlPartial* __restrict__ partials) {
  extern __shared__ __align__(16) unsigned char bl_smem[];
  __shared__ int s_code[BL_MAX_ROWS + 1];
  __shared__ float s_cls[BL_MAX_ROWS], s_box[BL_MAX_ROWS];
  __shared__ int s_flag[BL_MAX_ROWS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = p.K, C = p.C;
  const int r0 = blockIdx.x * p.rpw, nrows = min(p.rpw, p.R - r0);
  bl_stage_codes(gt_classes, p, r0, nrows, s_code);
  if (tid < BL_MAX_ROWS) { s_cls[tid] = 0.f; s_box[tid] = 0.f; s_flag[tid] = 0; }
  __syncthreads();
  const T* x = scores + (long)r0 * C;
  const int count = nrows * C;
  T* s_x = reinterpret_cast<T*>(bl_smem) + (int)(((uintptr_t)x & 15u) / sizeof(T));
  bl_stage_in(x, count, vec != 0, C, s_code, s_x);
  __syncthreads();
  for (int r = wave; r < nrows; r += BL_WAVES) {
    const int code = s_code[r];  // (the same in the whole wave)
    if (code < 0) continue;
    const T* row = s_x + r * C;
    float m = -INFINITY, s = 0.f, acc = 0.f;
    int idx = C;
    for (int j = lane; j < C; j += 64) {
      const float v = to_f32(row[j]);
      if (SIG) {
        if (j < K) {
          const float e = __expf(-fabsf(v));
          const float bce = fmaxf(v, 0.f) - (j == code ? v : 0.f) + __logf(1.f + e);
          acc += class_weight != nullptr ? class_weight[j] * bce : bce;
        }
        if (v > m) { m = v; idx = j; }
      } else if (v > m) {  // (m = -inf at first: exp2(-inf) = 0 and s = 0)
        s = s * __expf(m - v) + 1.f;
        m = v; idx = j;
      } else {
        s += __expf(v - m);
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {  // symmetric in the two lanes: every lane ends with the same bits
      const float m2 = bl_shfl(m, o);
      const int i2 = __shfl_xor(idx, o, 64);
      if (!SIG) {
        const float s2 = bl_shfl(s, o), M = fmaxf(m, m2);
        const float a = s * (m == M ? 1.f : __expf(m - M)), b = s2 * (m2 == M ? 1.f : __expf(m2 - M));
        s = a + b;
      }
      if (m2 > m || (m2 == m && i2 < idx)) idx = i2;
      m = fmaxf(m, m2);
    }
    if (SIG) acc = dl_wave_sum(acc);
    if (lane == 0) {
      if (!SIG) {
        acc = __logf(s) - (to_f32(row[code]) - m);
        rows_out[r0 + r] = BlRow{m, s};
      }
      s_cls[r] = acc;
      const int fg = code < K, hit = idx == code;
      s_flag[r] = 1 | (fg << 1) | (hit << 2) | ((fg & hit) << 3) | ((fg & (idx == K)) << 4);
    }
  }
  if (tid < nrows) {
    const int code = s_code[tid];
    if (code >= 0 && code < K) {
      float g[4];
      s_box[tid] = bl_box_row<T>(p, r0 + tid, code, deltas, boxes, gt_boxes, gt_index, gt_offsets, g);
    }
  }
  __syncthreads();
  if (tid == 0) {
    BlPartial o{};
    for (int r = 0; r < nrows; r++) {  // fixed order
      o.cls += s_cls[r];
      o.box += s_box[r];
      const int f = s_flag[r];
#pragma unroll
      for (int q = 0; q < 5; q++) o.n[q] += (f >> q) & 1;
    }
    partials[blockIdx.x] = o;
  }
}

// records -> loss_out[2] (divided by the rows that count), stats[5], and the count for the backward
__global__ __launch_bounds__(256) void d2amd_box_loss_final_kernel(const BlPartial* __restrict__ partials, int n,
                                                                  float* __restrict__ loss_out,
                                                                  int64_t* __restrict__ stats,
                                                                  int64_t* __restrict__ count_out) {
  const int tid = threadIdx.x;
  double c = 0., b = 0.;
  int k[5] = {0, 0, 0, 0, 0};
  for (int i = tid; i < n; i += 256) {
    const BlPartial v = partials[i];
    c += (double)v.cls; b += (double)v.box;
#pragma unroll
    for (int q = 0; q < 5; q++) k[q] += v.n[q];
  }
  __shared__ double sc[256], sb[256];
  __shared__ int sk[5][256];
  sc[tid] = c; sb[tid] = b;
#pragma unroll
  for (int q = 0; q < 5; q++) sk[q][tid] = k[q];
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {  // fixed tree: deterministic
    if (tid < s) {
      sc[tid] += sc[tid + s]; sb[tid] += sb[tid + s];
#pragma unroll
      for (int q = 0; q < 5; q++) sk[q][tid] += sk[q][tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const int rows = sk[0][0];
    loss_out[0] = rows > 0 ? (float)(sc[0] / (double)rows) : 0.f;
    loss_out[1] = rows > 0 ? (float)(sb[0] / (double)rows) : 0.f;
#pragma unroll
    for (int q = 0; q < 5; q++) stats[q] = sk[q][0];
    *count_out = rows;
  }
}

// ---- backward --------------------------------------------------------------------------------------------------
template <typename T, bool SIG>
__global__ __launch_bounds__(BL_THREADS) void d2amd_box_loss_backward_kernel(
    BlParams p, const T* __restrict__ scores, const T* __restrict__ deltas, const int64_t* __restrict__ gt_classes,
    const float* __restrict__ boxes, const float* __restrict__ gt_boxes, const int64_t* __restrict__ gt_index,
    const int64_t* __restrict__ gt_offsets, const float* __restrict__ class_weight, const float* __restrict__ grad_cls,
    const float* __restrict__ grad_box, const int64_t* __restrict__ count_in, const BlRow* __restrict__ rows_in, int vec,
    int vec_d, T* __restrict__ grad_scores, T* __restrict__ grad_deltas) {
  extern __shared__ __align__(16) unsigned char bl_smem[];
  __shared__ int s_code[BL_MAX_ROWS + 1];
  __shared__ float s_gd[BL_MAX_ROWS + 1][4];  // (+ 1: the streaming loop may step one row past the end before it stops)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = p.K, C = p.C, D = p.D;
  const int r0 = blockIdx.x * p.rpw, nrows = min(p.rpw, p.R - r0);
  bl_stage_codes(gt_classes, p, r0, nrows, s_code);
  if (tid < (BL_MAX_ROWS + 1) * 4) s_gd[tid >> 2][tid & 3] = 0.f;
  __syncthreads();
  const long rows = *count_in;
  const float inv = 1.f / (float)(rows > 0 ? rows : 1);
  const float gc = *grad_cls * inv, gb = *grad_box * inv;
  const T* x = scores + (long)r0 * C;
  const int count = nrows * C;
  T* s_x = reinterpret_cast<T*>(bl_smem) + (int)(((uintptr_t)x & 15u) / sizeof(T));
  bl_stage_in(x, count, vec != 0, C, s_code, s_x);
  if (tid < nrows) {  // the box gradient of the foreground rows -> LDS
    const int code = s_code[tid];
    if (code >= 0 && code < K) {
      float g[4];
      bl_box_row<T>(p, r0 + tid, code, deltas, boxes, gt_boxes, gt_index, gt_offsets, g);
#pragma unroll
      for (int i = 0; i < 4; i++) s_gd[tid][i] = g[i] * gb;
    }
  }
  __syncthreads();
  for (int r = wave; r < nrows; r += BL_WAVES) {  // the row's gradient replaces it in LDS
    const int code = s_code[r];
    T* row = s_x + r * C;
    if (code < 0) {
      for (int j = lane; j < C; j += 64) row[j] = from_f32<T>(0.f);
      continue;
    }
    if (SIG) {
      for (int j = lane; j < C; j += 64) {
        const float v = to_f32(row[j]);
        const float e = __expf(-fabsf(v));
        const float q = 1.f / (1.f + e);
        const float sg = v >= 0.f ? q : e * q;
        const float w = class_weight != nullptr && j < K ? class_weight[j] : 1.f;
        row[j] = from_f32<T>(j < K ? (sg - (j == code ? 1.f : 0.f)) * w * gc : 0.f);
      }
    } else {
      const BlRow rw = rows_in[r0 + r];
      const float is = 1.f / rw.s;
      for (int j = lane; j < C; j += 64) {
        const float v = to_f32(row[j]);
        row[j] = from_f32<T>((__expf(v - rw.m) * is - (j == code ? 1.f : 0.f)) * gc);
      }
    }
  }
  __syncthreads();
  bl_stage_out(s_x, count, vec != 0, grad_scores + (long)r0 * C);
  // the delta gradient: zeros, but the four entries of a foreground row's class (s_gd is zero for every other row)
  constexpr int V = dl_vec<T>::N;
  T* gd = grad_deltas + (long)r0 * D;
  const int cd = nrows * D;
  const int head = dl_head(gd, cd, vec_d != 0);
  const int nvec = (cd - head) / V, tail0 = head + nvec * V;
  auto entry = [&](int a, int c) -> float { return D == 4 || (c >> 2) == s_code[a] ? s_gd[a][c & 3] : 0.f; };
  for (int j = tid; j < head; j += BL_THREADS) {
    const int a = j / D;
    gd[j] = from_f32<T>(entry(a, j - a * D));
  }
  for (int i = tid; i < nvec; i += BL_THREADS) {
    float e[V];
    const int j0 = head + i * V;
    int a = j0 / D, c = j0 - a * D;
#pragma unroll
    for (int q = 0; q < V; q++) {
      e[q] = entry(a, c);
      const bool wrap = ++c == D;
      c = wrap ? 0 : c;
      a += wrap;
    }
    dl_store16(gd + j0, e);
  }
  for (int j = tail0 + tid; j < cd; j += BL_THREADS) {
    const int a = j / D;
    gd[j] = from_f32<T>(entry(a, j - a * D));
  }
}

}  // namespace d2amd

using namespace d2amd;

static size_t bl_workspace_bytes(long R) {
  return BL_HEADER_BYTES + (size_t)(R > 0 ? R : 0) * (sizeof(BlRow) + sizeof(BlPartial));
}

// argument checks shared by the two entries (everything but the outputs); fills p, the rows per workgroup included
static int bl_setup(const char* op, const void* scores, const void* deltas, const int64_t* gt_classes,
                    const float* proposal_boxes, const float* gt_boxes, const int64_t* gt_index, const int64_t* gt_offsets,
                    int R, int K, int delta_cols, int rows_per_image, int num_images, int gt_rows, int dtype, int cls_loss,
                    int box_loss, float beta, const float* weights, float scale_clamp, BlParams& p) {
  D2_CHECK_ARG(R >= 0 && K >= 1, "%s: bad shape (R %d, K %d)", op, R, K);
  D2_CHECK_ARG(dtype == D2AMD_F32 || dtype == D2AMD_F16 || dtype == D2AMD_BF16, "%s: unknown dtype %d", op, dtype);
  D2_CHECK_ARG(cls_loss == D2AMD_CLS_LOSS_SOFTMAX || cls_loss == D2AMD_CLS_LOSS_SIGMOID,
               "%s: classification loss %d (softmax 0, sigmoid 1)", op, cls_loss);
  D2_CHECK_ARG(box_loss == D2AMD_BOX_LOSS_SMOOTH_L1 || box_loss == D2AMD_BOX_LOSS_GIOU,
               "%s: box loss %d (smooth_l1 0, giou 1; diou / ciou are not implemented)", op, box_loss);
  const size_t es = dtype_size(dtype);
  D2_CHECK_ARG(((size_t)K + 1) * es + 32 <= BL_LDS_BYTES, "%s: K %d: a row of scores does not fit %zu bytes of LDS", op, K,
               BL_LDS_BYTES);
  D2_CHECK_ARG(delta_cols == 4 || (long)delta_cols == 4l * K, "%s: delta_cols %d is neither 4 nor 4 K = %ld", op,
               delta_cols, 4l * K);
  D2_CHECK_ARG((long)R * (K + 1) < (1l << 40) && beta >= 0.f, "%s: R * (K + 1) too large or beta %g < 0", op, beta);
  D2_CHECK_ARG(weights && weights[0] > 0.f && weights[1] > 0.f && weights[2] > 0.f && weights[3] > 0.f,
               "%s: box weights must be positive", op);
  if (R > 0) {
    D2_CHECK_ARG(scores && deltas && gt_classes && proposal_boxes && gt_boxes, "%s: null pointer", op);
    if (gt_index != nullptr)
      D2_CHECK_ARG(gt_offsets && rows_per_image >= 1 && num_images >= 1 && gt_rows >= 1 &&
                       (long)num_images * rows_per_image >= R,
                   "%s: the gt_index form needs gt_offsets, rows_per_image %d * num_images %d >= R %d and a table (%d rows)",
                   op, rows_per_image, num_images, R, gt_rows);
  }
  p = BlParams{};
  p.R = R; p.K = K; p.C = K + 1; p.D = delta_cols;
  p.S = rows_per_image; p.N = num_images; p.G = gt_rows;
  p.giou = box_loss == D2AMD_BOX_LOSS_GIOU; p.beta = beta;
  p.wx = weights[0]; p.wy = weights[1]; p.ww = weights[2]; p.wh = weights[3]; p.scale_clamp = scale_clamp;
  int rpw = BL_MAX_ROWS;
  const auto lds = [&](int rows) { return (size_t)rows * p.C * es + 32; };
  while (rpw > BL_WAVES && (lds(rpw) > BL_LDS_BYTES || cdiv(R, rpw) < 256)) rpw >>= 1;
  while (rpw > 1 && lds(rpw) > BL_LDS_BYTES) rpw >>= 1;
  p.rpw = rpw;
  return D2AMD_OK;
}

#define BL_LAUNCH(kernel, sig, grid, lds, s, ...)                                                      \
  do {                                                                                                 \
    if (sig)                                                                                           \
      hipLaunchKernelGGL((kernel<scalar_t, true>), grid, dim3(BL_THREADS), lds, s, __VA_ARGS__);       \
    else                                                                                               \
      hipLaunchKernelGGL((kernel<scalar_t, false>), grid, dim3(BL_THREADS), lds, s, __VA_ARGS__);      \
  } while (0)

extern "C" size_t d2amd_fast_rcnn_loss_workspace_bytes(int R) { return bl_workspace_bytes(R); }

extern "C" int d2amd_fast_rcnn_loss_forward(const void* scores, const void* deltas, const int64_t* gt_classes,
                                            const float* proposal_boxes, const float* gt_boxes, const int64_t* gt_index,
                                            const int64_t* gt_offsets, int R, int K, int delta_cols, int rows_per_image,
                                            int num_images, int gt_rows, int dtype, int cls_loss,
                                            const float* class_weight, int box_loss, float smooth_l1_beta,
                                            const float* weights, float scale_clamp, float* loss_out, int64_t* stats_out,
                                            void* workspace, size_t workspace_bytes, void* stream) {
  const char* op = "fast_rcnn_loss_forward";
  BlParams p;
  int rc = bl_setup(op, scores, deltas, gt_classes, proposal_boxes, gt_boxes, gt_index, gt_offsets, R, K, delta_cols,
                    rows_per_image, num_images, gt_rows, dtype, cls_loss, box_loss, smooth_l1_beta, weights, scale_clamp, p);
  if (rc) return rc;
  if (R == 0) return D2AMD_OK;  // nothing is launched: the caller's losses are zeros
  D2_CHECK_ARG(loss_out && stats_out, "%s: null output", op);
  D2_CHECK_ARG(workspace && ((uintptr_t)workspace & 7) == 0 && workspace_bytes >= bl_workspace_bytes(R),
               "%s: workspace missing, not 8-byte aligned or too small (%zu bytes, %zu needed)", op, workspace_bytes,
               bl_workspace_bytes(R));
  hipStream_t s = (hipStream_t)stream;
  int64_t* count = (int64_t*)workspace;
  BlRow* rows = (BlRow*)((char*)workspace + BL_HEADER_BYTES);
  BlPartial* partials = (BlPartial*)(rows + R);
  const size_t es = dtype_size(dtype);
  const int groups = cdiv(R, p.rpw);
  const size_t lds = (size_t)p.rpw * p.C * es + 32;
  const int vec = ((uintptr_t)scores % es) == 0;
  const bool sig = cls_loss == D2AMD_CLS_LOSS_SIGMOID;
  rc = D2_DISPATCH_DTYPE(dtype, [&]() -> int {
    BL_LAUNCH(d2amd_box_loss_forward_kernel, sig, dim3((unsigned)groups), lds, s, p, (const scalar_t*)scores,
              (const scalar_t*)deltas, gt_classes, proposal_boxes, gt_boxes, gt_index, gt_offsets, class_weight, vec, rows,
              partials);
    D2_LAUNCH_OK();
    return D2AMD_OK;
  });
  if (rc) return rc;
  hipLaunchKernelGGL(d2amd_box_loss_final_kernel, dim3(1), dim3(256), 0, s, partials, groups, loss_out, stats_out, count);
  D2_LAUNCH_OK();
  return D2AMD_OK;
}

extern "C" int d2amd_fast_rcnn_loss_backward(const void* scores, const void* deltas, const int64_t* gt_classes,
                                             const float* proposal_boxes, const float* gt_boxes, const int64_t* gt_index,
                                             const int64_t* gt_offsets, const float* grad_cls, const float* grad_box,
                                             int R, int K, int delta_cols, int rows_per_image, int num_images, int gt_rows,
                                             int dtype, int cls_loss, const float* class_weight, int box_loss,
                                             float smooth_l1_beta, const float* weights, float scale_clamp,
                                             const void* workspace, size_t workspace_bytes, void* grad_scores,
                                             void* grad_deltas, void* stream) {
  const char* op = "fast_rcnn_loss_backward";
  BlParams p;
  int rc = bl_setup(op, scores, deltas, gt_classes, proposal_boxes, gt_boxes, gt_index, gt_offsets, R, K, delta_cols,
                    rows_per_image, num_images, gt_rows, dtype, cls_loss, box_loss, smooth_l1_beta, weights, scale_clamp, p);
  if (rc) return rc;
  if (R == 0) return D2AMD_OK;
  D2_CHECK_ARG(grad_cls && grad_box && grad_scores && grad_deltas, "%s: null pointer", op);
  D2_CHECK_ARG(workspace && ((uintptr_t)workspace & 7) == 0 && workspace_bytes >= bl_workspace_bytes(R),
               "%s: workspace missing, not 8-byte aligned or too small (%zu bytes, %zu needed)", op, workspace_bytes,
               bl_workspace_bytes(R));
  hipStream_t s = (hipStream_t)stream;
  const int64_t* count = (const int64_t*)workspace;
  const BlRow* rows = (const BlRow*)((const char*)workspace + BL_HEADER_BYTES);
  const size_t es = dtype_size(dtype);
  const int groups = cdiv(R, p.rpw);
  const size_t lds = (size_t)p.rpw * p.C * es + 32;
  // 16-byte vectors through LDS need the scores and their gradient at the same offset inside 16 bytes, on an element
  // boundary (else the span moves by element)
  const int vec = (((uintptr_t)scores ^ (uintptr_t)grad_scores) & 15) == 0 && ((uintptr_t)scores % es) == 0;
  const int vec_d = ((uintptr_t)grad_deltas % es) == 0;
  const bool sig = cls_loss == D2AMD_CLS_LOSS_SIGMOID;
  return D2_DISPATCH_DTYPE(dtype, [&]() -> int {
    BL_LAUNCH(d2amd_box_loss_backward_kernel, sig, dim3((unsigned)groups), lds, s, p, (const scalar_t*)scores,
              (const scalar_t*)deltas, gt_classes, proposal_boxes, gt_boxes, gt_index, gt_offsets, class_weight, grad_cls,
              grad_box, count, rows, vec, vec_d, (scalar_t*)grad_scores, (scalar_t*)grad_deltas);
    D2_LAUNCH_OK();
    return D2AMD_OK;
  });
}
