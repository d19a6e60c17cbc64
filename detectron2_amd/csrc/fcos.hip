// Training head of FCOS, fused: point matching, sigmoid focal classification, GIoU through the linear box transform and
// the centerness BCE of ALL images and levels in one forward and one backward launch.
//   replaces  detectron2/modeling/meta_arch/fcos.py:97-191 (_match_anchors / label_anchors: per image an (M, R, 4) fp32
//             distance tensor, several (M, R) temporaries and a max over M),
//             fcos.py:193-251 (losses / compute_ctrness_targets: a one-hot the size of the logits, cat over the levels,
//             three boolean-mask gathers, `.item()` on the number of positives) and
//             detectron2/modeling/box_regression.py:230-307 (Box2BoxTransformLinear.get_deltas / apply_deltas).
// There is no contraction anywhere in this head, so the matrix units (MFMA) have nothing to do: the work is LDS
// staging, streaming 16-byte loads and register math.
// Here:
//   * a WORKGROUP (256 threads) OWNS A TILE of FC_TILE = 256 consecutive anchor points of one (image, level), as
//     dense_loss.hip does; the level table is a by-value kernel argument, nothing is concatenated.
//       1. MATCHING.  Thread i owns point i.  The image's ground truth (packed [G, 4] boxes, offsets int32 [N + 1] ON THE
//          DEVICE) is staged in LDS in chunks of FC_GT_CHUNK = 128 boxes, 32 B each: thread j loads box j of the chunk
//          once and stores the corners, the centre and the quality 1e8f - area; every thread then scans the chunk (all
//          lanes read the same entry: two broadcast 16-byte LDS reads per pair).  128 boxes are 4 KB of LDS, leave eight
//          workgroups per CU resident and cover a COCO image (7 boxes on average, a few per cent above 32) in one pass;
//          a larger chunk buys nothing, the scan is one barrier pair per chunk either way.
//          The tests are the reference's in fp32 in its operation order (this file is built without FMA contraction):
//            max(|cx - gx|, |cy - gy|) < radius * size,  min(l, t, r, b) > 0,  lower < max(l, t, r, b) < upper,
//          size = x2 - x1 of the point's own anchor, lower = 4 size (0 on the first level), upper = 8 size (+inf on the
//          last).  The winner is the largest fp32 quality, the lowest index among equals (torch's first maximum); a
//          quality < 1e-5 (an area above 1e8) never matches.  The matched box stays in the owner's registers, the class
//          code goes to LDS, `matched` (int32, -1 background) is written once: all the backward needs.
//       2. CLASSIFICATION.  The tile's cnt * K contiguous logits are streamed with 16-byte loads (head / tail by
//          element, as in dense_loss.hip); the focal term (loss_common.h) takes its target from the LDS code.
//       3. BOX AND CENTERNESS of the tile's positives, in their owning threads: relu(delta) (* anchor size), corners
//          cx - l, cy - t, cx + r, cy + b, GIoU with eps 1e-7 against the matched box, gradient through the relu (0 for
//          delta <= 0); centerness target sqrt(min(l,r)/max(l,r) * min(t,b)/max(t,b)) of get_deltas(anchor, matched
//          box), BCE with logits max(x,0) - x t + log1p(exp(-|x|)), gradient sigmoid(x) - t.
//   * reductions: butterfly inside a wave, four waves added in order, one (cls, loc, ctr, #pos) record per tile; a
//     one-workgroup kernel adds the records in fp64 in a fixed order.  No float atomics: bit-identical runs.
//   * backward: same tiling, targets from `matched` (or the given labels / boxes), the three upstream gradients from
//     device scalars, everything recomputed from the inputs; EVERY element of every level's logit, delta and centerness
//     gradient is written exactly once, zeros included.
//   * the targets may also be GIVEN (gt_labels [N, R], gt_boxes [N, R, 4]: FCOS.losses' own arguments): same kernels,
//     same arithmetic, the matching replaced by two loads.
// Nothing reads the host; the offsets are device data, so a captured graph replays with other ground-truth counts.
#include <math.h>

#include "common.h"
#include "loss_common.h"

namespace d2amd {

constexpr int FC_TILE = 256;     // anchor points per workgroup
constexpr int FC_THREADS = 256;  // == FC_TILE: thread i owns point i of the tile
constexpr int FC_MAX_LEVELS = D2AMD_RPN_MAX_LEVELS;
constexpr int FC_GT_CHUNK = D2AMD_FCOS_GT_CHUNK;  // ground-truth boxes staged in LDS at a time
static_assert(FC_GT_CHUNK <= FC_THREADS, "one staging thread per box of a chunk");

struct FcLevels {
  const void* logits[FC_MAX_LEVELS];   // [N, A_l, K]
  const void* deltas[FC_MAX_LEVELS];   // [N, A_l, 4]
  const void* ctr[FC_MAX_LEVELS];      // [N, A_l]
  const float* anchors[FC_MAX_LEVELS]; // [A_l, 4]
  void* glogits[FC_MAX_LEVELS];        // backward only
  void* gdeltas[FC_MAX_LEVELS];
  void* gctr[FC_MAX_LEVELS];
  int A[FC_MAX_LEVELS];
  int aoff[FC_MAX_LEVELS];             // prefix of A_l: the level's first column of the [N, R] arrays
  int tile_base[FC_MAX_LEVELS + 1];    // prefix of N * cdiv(A_l, FC_TILE); entries behind L repeat the total
  int L;
};

struct FcParams {
  int N, K, R, G;  // G: rows of the packed ground truth (the device offsets are clamped to it)
  float alpha, gamma, radius;
  int norm;        // Box2BoxTransformLinear.normalize_by_size
};

// where a point's target comes from
enum { FC_SRC_MATCH = 0, FC_SRC_INDEX = 1, FC_SRC_GIVEN = 2 };
struct FcTargets {
  const float* gt_boxes;      // packed [G, 4]                      (MATCH, INDEX)
  const int64_t* gt_classes;  // packed [G]
  const int* gt_offsets;      // [N + 1]
  int* matched;               // [N, R]: written by MATCH, read by INDEX
  const int64_t* labels;      // [N, R]                              (GIVEN)
  const float* boxes;         // [N, R, 4]
};

struct FcPartial { float cls, loc, ctr; int pos; };  // one per tile

// ---- the tile of a workgroup -------------------------------------------------------------------------------------
struct FcTile {
  const void* logits; const void* deltas; const void* ctr; const float* anchors;
  void* glogits; void* gdeltas; void* gctr;
  int A, col0, n, a0, cnt;  // col0: column of point a0 in the [N, R] arrays
  bool first, last;         // level 0 / level L - 1: no lower / no upper bound on the regression range
};

__device__ __forceinline__ FcTile fc_tile(const FcLevels& P, int b) {
  int l = 0;
#pragma unroll
  for (int q = 1; q < FC_MAX_LEVELS; q++)
    if (q < P.L && b >= P.tile_base[q]) l = q;
  FcTile t{};
  int base = 0, aoff = 0;
#pragma unroll
  for (int q = 0; q < FC_MAX_LEVELS; q++)  // (selects: no runtime index into the by-value argument)
    if (q == l) {
      t.logits = P.logits[q]; t.deltas = P.deltas[q]; t.ctr = P.ctr[q]; t.anchors = P.anchors[q];
      t.glogits = P.glogits[q]; t.gdeltas = P.gdeltas[q]; t.gctr = P.gctr[q];
      t.A = P.A[q]; aoff = P.aoff[q]; base = P.tile_base[q];
    }
  const int per_image = (t.A + FC_TILE - 1) / FC_TILE;
  const int r = b - base;
  t.n = r / per_image;
  t.a0 = (r - t.n * per_image) * FC_TILE;
  t.cnt = min(FC_TILE, t.A - t.a0);
  t.col0 = aoff + t.a0;
  t.first = l == 0;
  t.last = l == P.L - 1;
  return t;
}

__device__ __forceinline__ void fc_load4(const float* p, float (&o)[4]) {
  const float4 v = *reinterpret_cast<const float4*>(p);
  o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
}

// rows [off0, off0 + count) of the packed ground truth belong to image n (clamped: the offsets are device data)
__device__ __forceinline__ int2 fc_gt_range(const int* __restrict__ gt_offsets, int n, int G) {
  const int lo = min(max(gt_offsets[n], 0), G), hi = min(max(gt_offsets[n + 1], lo), G);
  return make_int2(lo, hi - lo);
}

// ---- 1. matching (fcos.py:113-151, 171-172) -----------------------------------------------------------------------
// Called by the whole workgroup (barriers inside); `active` threads own a point with anchor `an`.
// -> index of the matched box inside the image's ground truth or -1, the box itself in mb
__device__ __forceinline__ int fc_match(const float* __restrict__ gt_boxes, int off0, int count, bool active,
                                        const float (&an)[4], bool first, bool last, float radius, float4* s_box,
                                        float4* s_aux, float (&mb)[4]) {
  const int tid = threadIdx.x;
  const float cx = (an[0] + an[2]) / 2.f, cy = (an[1] + an[3]) / 2.f;  // Boxes.get_centers
  const float size = an[2] - an[0];
  const float lower = first ? 0.f : size * 4.f;
  const float upper = last ? INFINITY : size * 8.f;
  const float reach = radius * size;
  int best = -1;
  float bestq = 0.f;  // a point no box passes has quality 0
  for (int c0 = 0; c0 < count; c0 += FC_GT_CHUNK) {  // (count is the same in every thread)
    const int m = min(FC_GT_CHUNK, count - c0);
    __syncthreads();  // the previous chunk has been scanned
    if (tid < m) {
      const float4 b = *reinterpret_cast<const float4*>(gt_boxes + (long)(off0 + c0 + tid) * 4);
      s_box[tid] = b;
      s_aux[tid] = make_float4((b.x + b.z) / 2.f, (b.y + b.w) / 2.f, 1e8f - (b.z - b.x) * (b.w - b.y), 0.f);
    }
    __syncthreads();
    if (active)
      for (int j = 0; j < m; j++) {
        const float4 b = s_box[j], a = s_aux[j];
        const float dx = fabsf(cx - a.x), dy = fabsf(cy - a.y);
        const float l = cx - b.x, t = cy - b.y, r = b.z - cx, d = b.w - cy;  // pairwise_point_box_distance
        const float lo = fminf(fminf(l, t), fminf(r, d)), hi = fmaxf(fmaxf(l, t), fmaxf(r, d));
        const bool ok = fmaxf(dx, dy) < reach && lo > 0.f && hi > lower && hi < upper;
        if (ok && a.z > bestq) {  // strictly larger: the first of equal qualities stays
          bestq = a.z;
          best = c0 + j;
          mb[0] = b.x; mb[1] = b.y; mb[2] = b.z; mb[3] = b.w;
        }
      }
  }
  return bestq < 1e-5f ? -1 : best;
}

// class code of a target class: c < K positive of class c, K background (FCOS ignores no point)
__device__ __forceinline__ int fc_code(int64_t v, int K) { return v >= 0 && v < K ? (int)v : K; }

// -> the class code of the thread's point (-1 behind the tile's end), its target box in mb when the code is positive
template <int SRC>
__device__ __forceinline__ int fc_target(const FcTargets& g, const FcParams& p, const FcTile& t, const float (&an)[4],
                                         float4* s_box, float4* s_aux, float (&mb)[4]) {
  const int tid = threadIdx.x;
  const bool active = tid < t.cnt;
  const long col = (long)t.n * p.R + t.col0 + tid;
  int code = p.K;
  if (SRC == FC_SRC_GIVEN) {
    if (active) {
      code = fc_code(g.labels[col], p.K);
      if (code < p.K) fc_load4(g.boxes + col * 4, mb);
    }
  } else {
    const int2 range = fc_gt_range(g.gt_offsets, t.n, p.G);
    int idx = -1;
    if (SRC == FC_SRC_MATCH) {
      idx = fc_match(g.gt_boxes, range.x, range.y, active, an, t.first, t.last, p.radius, s_box, s_aux, mb);
      if (active) g.matched[col] = idx;
    } else if (active) {
      idx = g.matched[col];
      if (idx >= range.y) idx = -1;
      if (idx >= 0) fc_load4(g.gt_boxes + (long)(range.x + idx) * 4, mb);
    }
    if (active && idx >= 0) code = fc_code(g.gt_classes[range.x + idx], p.K);
  }
  return active ? code : -1;
}

// ---- 3. box and centerness of one positive point -----------------------------------------------------------------
// d: the point's four predicted deltas, x: its centerness logit.
// -> loc / ctr losses; gd = d loc / d delta, gc = d ctr / d x
__device__ __forceinline__ void fc_point_terms(const float (&an)[4], const float (&gt)[4], const float (&d)[4], float x,
                                               bool norm, float& loc, float& ctr, float (&gd)[4], float& gc) {
  const float sw = an[2] - an[0], sh = an[3] - an[1];
  const float cx = 0.5f * (an[0] + an[2]), cy = 0.5f * (an[1] + an[3]);
  const float kx = norm ? sw : 1.f, ky = norm ? sh : 1.f;
  // Box2BoxTransformLinear.apply_deltas, then fvcore giou_loss
  const float el = fmaxf(d[0], 0.f) * kx, et = fmaxf(d[1], 0.f) * ky, er = fmaxf(d[2], 0.f) * kx, eb = fmaxf(d[3], 0.f) * ky;
  float g[4];
  loc = dl_giou_corners<float>(cx - el, cy - et, cx + er, cy + eb, gt, g);
  gd[0] = d[0] > 0.f ? -g[0] * kx : 0.f;  // relu: no gradient at or below 0
  gd[1] = d[1] > 0.f ? -g[1] * ky : 0.f;
  gd[2] = d[2] > 0.f ? g[2] * kx : 0.f;
  gd[3] = d[3] > 0.f ? g[3] * ky : 0.f;
  // compute_ctrness_targets on get_deltas(anchor, matched box)
  float l = cx - gt[0], t = cy - gt[1], r = gt[2] - cx, b = gt[3] - cy;
  if (norm) { l /= sw; t /= sh; r /= sw; b /= sh; }
  const float tg = sqrtf((fminf(l, r) / fmaxf(l, r)) * (fminf(t, b) / fmaxf(t, b)));
  const float e = expf(-fabsf(x));
  ctr = fmaxf(x, 0.f) - x * tg + log1pf(e);
  gc = (x >= 0.f ? 1.f / (1.f + e) : e / (1.f + e)) - tg;
}

template <typename T> __device__ __forceinline__ void fc_load_row(const T* p, float (&o)[4]) {
  unpack4(*reinterpret_cast<const vec4<T>*>(p), o);  // (rows are 4 * sizeof(T)-aligned: checked on the host)
}

// ---- forward ---------------------------------------------------------------------------------------------------
template <typename T, int GM, int SRC>
__global__ __launch_bounds__(FC_THREADS) void d2amd_fcos_loss_forward_kernel(FcLevels P, FcParams p, FcTargets g, int vec,
                                                                             FcPartial* __restrict__ partials) {
  __shared__ float4 s_box[FC_GT_CHUNK], s_aux[FC_GT_CHUNK];
  __shared__ int s_lab[FC_TILE + 1];  // (+ 1: the streaming loop may step one point past the tile before it stops)
  __shared__ int s_pos;
  __shared__ float s_red[FC_THREADS / 64][3];
  const int tid = threadIdx.x;
  const FcTile t = fc_tile(P, blockIdx.x);
  float an[4] = {0.f, 0.f, 0.f, 0.f}, mb[4] = {0.f, 0.f, 0.f, 0.f};
  if (tid < t.cnt) fc_load4(t.anchors + (long)(t.a0 + tid) * 4, an);
  const int code = fc_target<SRC>(g, p, t, an, s_box, s_aux, mb);
  const bool positive = code >= 0 && code < p.K;
  s_lab[tid] = code;
  if (tid == 0) { s_lab[FC_TILE] = -1; s_pos = 0; }
  __syncthreads();
  const int wave_pos = __popcll(__ballot(positive));
  if ((tid & 63) == 0) atomicAdd(&s_pos, wave_pos);  // integers: order-independent

  // 2. classification: every point is valid
  float cls = 0.f, loc = 0.f, ctr = 0.f;
  {
    constexpr int V = dl_vec<T>::N;
    const int K = p.K, count = t.cnt * K;
    const T* x = (const T*)t.logits + ((long)t.n * t.A + t.a0) * K;
    const int head = dl_head(x, count, vec != 0);
    const int nvec = (count - head) / V, tail0 = head + nvec * V;
    for (int j = tid; j < head; j += FC_THREADS) {
      const int a = j / K;
      cls += dl_focal<GM>(to_f32(x[j]), s_lab[a], j - a * K, p);
    }
    for (int i = tid; i < nvec; i += FC_THREADS) {
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
    const int j = tail0 + tid;
    if (j < count) {
      const int a = j / K;
      cls += dl_focal<GM>(to_f32(x[j]), s_lab[a], j - a * K, p);
    }
  }
  // 3. box + centerness: the centerness logits are read one per thread, coalesced
  if (tid < t.cnt) {
    const long row = (long)t.n * t.A + t.a0 + tid;
    const float xc = to_f32(((const T*)t.ctr)[row]);
    if (positive) {
      float d[4], gd[4], gc;
      fc_load_row((const T*)t.deltas + row * 4, d);
      fc_point_terms(an, mb, d, xc, p.norm != 0, loc, ctr, gd, gc);
    }
  }
  cls = dl_wave_sum(cls);
  loc = dl_wave_sum(loc);
  ctr = dl_wave_sum(ctr);
  if ((tid & 63) == 0) { s_red[tid >> 6][0] = cls; s_red[tid >> 6][1] = loc; s_red[tid >> 6][2] = ctr; }
  __syncthreads();
  if (tid == 0) {
    FcPartial o;
    o.cls = ((s_red[0][0] + s_red[1][0]) + s_red[2][0]) + s_red[3][0];  // fixed order
    o.loc = ((s_red[0][1] + s_red[1][1]) + s_red[2][1]) + s_red[3][1];
    o.ctr = ((s_red[0][2] + s_red[1][2]) + s_red[2][2]) + s_red[3][2];
    o.pos = s_pos;
    partials[blockIdx.x] = o;
  }
}

__global__ __launch_bounds__(256) void d2amd_fcos_loss_final_kernel(const FcPartial* __restrict__ partials, int tiles,
                                                                   long points, float* __restrict__ loss_cls,
                                                                   float* __restrict__ loss_loc,
                                                                   float* __restrict__ loss_ctr,
                                                                   int64_t* __restrict__ stats) {
  const int tid = threadIdx.x;
  double c = 0., b = 0., q = 0.;
  long pos = 0;
  for (int i = tid; i < tiles; i += 256) {
    const FcPartial v = partials[i];
    c += (double)v.cls; b += (double)v.loc; q += (double)v.ctr; pos += v.pos;
  }
  __shared__ double sc[256], sb[256], sq[256];
  __shared__ long sp[256];
  sc[tid] = c; sb[tid] = b; sq[tid] = q; sp[tid] = pos;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {  // fixed tree: deterministic
    if (tid < s) { sc[tid] += sc[tid + s]; sb[tid] += sb[tid + s]; sq[tid] += sq[tid + s]; sp[tid] += sp[tid + s]; }
    __syncthreads();
  }
  if (tid == 0) {
    *loss_cls = (float)sc[0];
    *loss_loc = (float)sb[0];
    *loss_ctr = (float)sq[0];
    stats[0] = sp[0];
    stats[1] = points;
  }
}

// ---- backward --------------------------------------------------------------------------------------------------
template <typename T, int GM, int SRC>
__global__ __launch_bounds__(FC_THREADS) void d2amd_fcos_loss_backward_kernel(FcLevels P, FcParams p, FcTargets g,
                                                                              const float* __restrict__ grad_cls,
                                                                              const float* __restrict__ grad_loc,
                                                                              const float* __restrict__ grad_ctr,
                                                                              int vec) {
  __shared__ int s_lab[FC_TILE + 1];
  const int tid = threadIdx.x;
  const FcTile t = fc_tile(P, blockIdx.x);
  float an[4] = {0.f, 0.f, 0.f, 0.f}, mb[4] = {0.f, 0.f, 0.f, 0.f};
  if (tid < t.cnt) fc_load4(t.anchors + (long)(t.a0 + tid) * 4, an);
  const int code = fc_target<SRC>(g, p, t, an, nullptr, nullptr, mb);  // (INDEX / GIVEN: no staging)
  s_lab[tid] = code;
  if (tid == 0) s_lab[FC_TILE] = -1;
  __syncthreads();
  {
    constexpr int V = dl_vec<T>::N;
    const int K = p.K, count = t.cnt * K;
    const long e0 = ((long)t.n * t.A + t.a0) * K;
    const T* x = (const T*)t.logits + e0;
    T* gx = (T*)t.glogits + e0;
    const int head = dl_head(gx, count, vec != 0);  // (vec: logits and gradient share their offset inside 16 bytes)
    const int nvec = (count - head) / V, tail0 = head + nvec * V;
    const float up = *grad_cls;
    for (int j = tid; j < head; j += FC_THREADS) {
      const int a = j / K;
      gx[j] = from_f32<T>(dl_focal_grad<GM>(to_f32(x[j]), s_lab[a], j - a * K, p, up));
    }
    for (int i = tid; i < nvec; i += FC_THREADS) {
      float e[V];
      const int j0 = head + i * V;
      dl_load16(x + j0, e);
      int a = j0 / K, c = j0 - a * K;
#pragma unroll
      for (int q = 0; q < V; q++) {
        e[q] = dl_focal_grad<GM>(e[q], s_lab[a], c, p, up);
        const bool wrap = ++c == K;
        c = wrap ? 0 : c;
        a += wrap;
      }
      dl_store16(gx + j0, e);
    }
    const int j = tail0 + tid;
    if (j < count) {
      const int a = j / K;
      gx[j] = from_f32<T>(dl_focal_grad<GM>(to_f32(x[j]), s_lab[a], j - a * K, p, up));
    }
  }
  // the delta row and the centerness gradient of the thread's point: zeros unless it is positive
  if (tid < t.cnt) {
    const long row = (long)t.n * t.A + t.a0 + tid;
    float gd[4] = {0.f, 0.f, 0.f, 0.f}, gc = 0.f;
    if (code < p.K) {
      float d[4], loc, ctr;
      fc_load_row((const T*)t.deltas + row * 4, d);
      fc_point_terms(an, mb, d, to_f32(((const T*)t.ctr)[row]), p.norm != 0, loc, ctr, gd, gc);
      const float ul = *grad_loc;
#pragma unroll
      for (int i = 0; i < 4; i++) gd[i] *= ul;
      gc *= *grad_ctr;
    }
    vec4<T> o;
    pack4(gd, o);
    *reinterpret_cast<vec4<T>*>((T*)t.gdeltas + row * 4) = o;
    ((T*)t.gctr)[row] = from_f32<T>(gc);
  }
}

// ---- label_anchors: the matching alone, in the reference's output form --------------------------------------------
__global__ __launch_bounds__(FC_THREADS) void d2amd_fcos_label_anchors_kernel(FcLevels P, FcParams p, FcTargets g,
                                                                              int64_t* __restrict__ labels,
                                                                              float* __restrict__ boxes) {
  __shared__ float4 s_box[FC_GT_CHUNK], s_aux[FC_GT_CHUNK];
  const int tid = threadIdx.x;
  const FcTile t = fc_tile(P, blockIdx.x);
  const bool active = tid < t.cnt;
  float an[4] = {0.f, 0.f, 0.f, 0.f}, mb[4] = {0.f, 0.f, 0.f, 0.f};
  if (active) fc_load4(t.anchors + (long)(t.a0 + tid) * 4, an);
  const int2 range = fc_gt_range(g.gt_offsets, t.n, p.G);
  const int idx = fc_match(g.gt_boxes, range.x, range.y, active, an, t.first, t.last, p.radius, s_box, s_aux, mb);
  if (!active) return;
  const long col = (long)t.n * p.R + t.col0 + tid;
  // an unmatched point carries the image's box 0 (the reference's clip(min = 0)); no ground truth: a zero box
  if (idx < 0 && range.y > 0) fc_load4(g.gt_boxes + (long)range.x * 4, mb);
  labels[col] = idx >= 0 ? g.gt_classes[range.x + idx] : (int64_t)p.K;
  *reinterpret_cast<float4*>(boxes + col * 4) = make_float4(mb[0], mb[1], mb[2], mb[3]);
  if (g.matched) g.matched[col] = idx;
}

}  // namespace d2amd

using namespace d2amd;

// level table + shape checks shared by the entries; -> R and the number of tiles
static int fc_layout(const char* op, int N, const int* level_anchors, int L, int K, FcLevels& P, int* R, long* tiles) {
  D2_CHECK_ARG(N >= 0 && L >= 0 && L <= FC_MAX_LEVELS && (L == 0 || level_anchors) && K >= 1 && K < (1 << 22),
               "%s: bad shape (N %d, %d levels [max %d], K %d)", op, N, L, FC_MAX_LEVELS, K);
  P = FcLevels{};
  P.L = L;
  long r = 0, t = 0;
  for (int l = 0; l < L; l++) {
    D2_CHECK_ARG(level_anchors[l] >= 1 && (long)level_anchors[l] * K < (1l << 31),
                 "%s: level %d has %d anchor points (a level needs at least one; A * K < 2^31)", op, l, level_anchors[l]);
    P.A[l] = level_anchors[l];
    P.aoff[l] = (int)r;
    P.tile_base[l] = (int)t;
    r += level_anchors[l];
    t += (long)N * ((level_anchors[l] + FC_TILE - 1) / FC_TILE);
    D2_CHECK_ARG(r < (1l << 31) && t < (1l << 31) && (long)N * r < (1l << 40), "%s: too many anchor points", op);
  }
  for (int l = L; l <= FC_MAX_LEVELS; l++) P.tile_base[l] = (int)t;
  *R = (int)r;
  *tiles = t;
  return D2AMD_OK;
}

static int fc_params(const char* op, int N, int K, int R, int G, float radius, int normalize_by_size, float alpha,
                     float gamma, FcParams& p) {
  D2_CHECK_ARG(G >= 0 && radius == radius, "%s: %d ground-truth rows or a NaN sampling radius", op, G);
  D2_CHECK_ARG(gamma >= 0.f && gamma == gamma && alpha <= 1.f, "%s: gamma %g < 0 or alpha %g > 1", op, gamma, alpha);
  p.N = N; p.K = K; p.R = R; p.G = G;
  p.alpha = alpha; p.gamma = gamma; p.radius = radius; p.norm = normalize_by_size != 0;
  return D2AMD_OK;
}

// packed ground truth (gt_offsets is never null; boxes / classes may be when G == 0) or given targets
static int fc_targets(const char* op, const float* gt_boxes, const int64_t* gt_classes, const int* gt_offsets, int G,
                      int* matched, const int64_t* gt_labels, const float* matched_boxes, FcTargets& g, bool* given) {
  *given = gt_labels != nullptr || matched_boxes != nullptr;
  g = FcTargets{};
  if (*given) {
    D2_CHECK_ARG(gt_labels && matched_boxes && ((uintptr_t)matched_boxes & 15) == 0,
                 "%s: given targets need gt_labels and 16-byte aligned matched boxes", op);
    g.labels = gt_labels; g.boxes = matched_boxes;
    return D2AMD_OK;
  }
  D2_CHECK_ARG(gt_offsets && matched && (G == 0 || (gt_boxes && gt_classes)) && ((uintptr_t)gt_boxes & 15) == 0,
               "%s: packed ground truth needs 16-byte aligned gt_boxes, gt_classes, gt_offsets and `matched`", op);
  g.gt_boxes = gt_boxes; g.gt_classes = gt_classes; g.gt_offsets = gt_offsets; g.matched = matched;
  return D2AMD_OK;
}

// the three gamma variants of a kernel template for scalar_t and a target source
#define FC_LAUNCH_G(kernel, SRC, gamma, grid, s, ...)                                                                  \
  do {                                                                                                                 \
    if ((gamma) == 0.f)                                                                                                \
      hipLaunchKernelGGL((kernel<scalar_t, 0, SRC>), grid, dim3(FC_THREADS), 0, s, __VA_ARGS__);                       \
    else if ((gamma) == 2.f)                                                                                           \
      hipLaunchKernelGGL((kernel<scalar_t, 2, SRC>), grid, dim3(FC_THREADS), 0, s, __VA_ARGS__);                       \
    else                                                                                                               \
      hipLaunchKernelGGL((kernel<scalar_t, 1, SRC>), grid, dim3(FC_THREADS), 0, s, __VA_ARGS__);                       \
  } while (0)

extern "C" int d2amd_fcos_gt_chunk(void) { return FC_GT_CHUNK; }

extern "C" size_t d2amd_fcos_loss_workspace_bytes(int N, const int* level_anchors, int L) {
  FcLevels P; int R; long tiles;
  if (fc_layout("fcos_loss_workspace_bytes", N, level_anchors, L, 1, P, &R, &tiles)) return sizeof(FcPartial);
  return sizeof(FcPartial) * (size_t)(tiles > 0 ? tiles : 1);
}

extern "C" int d2amd_fcos_label_anchors(const float* const* anchors, const float* gt_boxes, const int64_t* gt_classes,
                                        const int* gt_offsets, int G, int N, const int* level_anchors, int L,
                                        int num_classes, float radius, int64_t* labels_out, float* boxes_out,
                                        int* matched_out, void* stream) {
  const char* op = "fcos_label_anchors";
  FcLevels P; FcParams p{}; FcTargets g{}; int R; long tiles;
  int rc = fc_layout(op, N, level_anchors, L, 1, P, &R, &tiles);
  if (rc) return rc;
  rc = fc_params(op, N, num_classes, R, G, radius, 1, 0.f, 0.f, p);
  if (rc) return rc;
  if (tiles == 0) return D2AMD_OK;
  D2_CHECK_ARG(anchors && gt_offsets && labels_out && boxes_out && (G == 0 || (gt_boxes && gt_classes)) &&
                   (((uintptr_t)gt_boxes | (uintptr_t)boxes_out) & 15) == 0,
               "%s: null pointer, or gt_boxes / boxes_out not 16-byte aligned", op);
  for (int l = 0; l < L; l++) {
    D2_CHECK_ARG(anchors[l] && ((uintptr_t)anchors[l] & 15) == 0, "%s: anchors[%d] null or not 16-byte aligned", op, l);
    P.anchors[l] = anchors[l];
  }
  g.gt_boxes = gt_boxes; g.gt_classes = gt_classes; g.gt_offsets = gt_offsets; g.matched = matched_out;
  hipLaunchKernelGGL(d2amd_fcos_label_anchors_kernel, dim3((unsigned)tiles), dim3(FC_THREADS), 0, (hipStream_t)stream, P,
                     p, g, labels_out, boxes_out);
  D2_LAUNCH_OK();
  return D2AMD_OK;
}

// the level pointers of forward (grads == false) and backward; -> *vec: 16-byte vectors on the logits are possible
static int fc_pointers(const char* op, int dtype, const void* const* logits, const void* const* deltas,
                       const void* const* ctrness, const float* const* anchors, void* const* grad_logits,
                       void* const* grad_deltas, void* const* grad_ctrness, bool grads, FcLevels& P, bool* vec) {
  D2_CHECK_ARG(dtype == D2AMD_F32 || dtype == D2AMD_F16 || dtype == D2AMD_BF16, "%s: unsupported dtype %d", op, dtype);
  D2_CHECK_ARG(logits && deltas && ctrness && anchors && (!grads || (grad_logits && grad_deltas && grad_ctrness)),
               "%s: null pointer", op);
  const size_t es = dtype_size(dtype);
  *vec = true;
  for (int l = 0; l < P.L; l++) {
    D2_CHECK_ARG(logits[l] && deltas[l] && ctrness[l] && anchors[l], "%s: null level %d", op, l);
    D2_CHECK_ARG(((uintptr_t)anchors[l] & 15) == 0 && ((uintptr_t)deltas[l] & (4 * es - 1)) == 0 &&
                     ((uintptr_t)ctrness[l] & (es - 1)) == 0,
                 "%s: level %d: anchors / deltas not aligned to a row of four, or centerness not to an element", op, l);
    P.logits[l] = logits[l]; P.deltas[l] = deltas[l]; P.ctr[l] = ctrness[l]; P.anchors[l] = anchors[l];
    *vec = *vec && ((uintptr_t)logits[l] % es) == 0;
    if (grads) {
      D2_CHECK_ARG(grad_logits[l] && grad_deltas[l] && grad_ctrness[l], "%s: null gradient of level %d", op, l);
      D2_CHECK_ARG(((uintptr_t)grad_deltas[l] & (4 * es - 1)) == 0 && ((uintptr_t)grad_ctrness[l] & (es - 1)) == 0 &&
                       ((uintptr_t)grad_logits[l] & (es - 1)) == 0,
                   "%s: level %d: grad_deltas not aligned to a row of four, or a gradient not to an element", op, l);
      P.glogits[l] = grad_logits[l]; P.gdeltas[l] = grad_deltas[l]; P.gctr[l] = grad_ctrness[l];
      // 16-byte vectors need the logits and their gradient at the same offset inside 16 bytes
      *vec = *vec && (((uintptr_t)logits[l] ^ (uintptr_t)grad_logits[l]) & 15) == 0;
    }
  }
  return D2AMD_OK;
}

extern "C" int d2amd_fcos_loss_forward(const void* const* logits, const void* const* deltas, const void* const* ctrness,
                                       const float* const* anchors, const float* gt_boxes, const int64_t* gt_classes,
                                       const int* gt_offsets, int G, const int64_t* gt_labels,
                                       const float* matched_boxes, int N, const int* level_anchors, int L, int K,
                                       int dtype, float radius, int normalize_by_size, float alpha, float gamma,
                                       int* matched_out, float* loss_cls_sum, float* loss_loc_sum, float* loss_ctr_sum,
                                       int64_t* stats, void* workspace, size_t workspace_bytes, void* stream) {
  const char* op = "fcos_loss_forward";
  FcLevels P; FcParams p{}; FcTargets g{}; int R; long tiles; bool given, vec;
  int rc = fc_layout(op, N, level_anchors, L, K, P, &R, &tiles);
  if (rc) return rc;
  rc = fc_params(op, N, K, R, G, radius, normalize_by_size, alpha, gamma, p);
  if (rc) return rc;
  D2_CHECK_ARG(loss_cls_sum && loss_loc_sum && loss_ctr_sum && stats, "%s: null output", op);
  const size_t need = sizeof(FcPartial) * (size_t)(tiles > 0 ? tiles : 1);
  D2_CHECK_ARG(workspace && ((uintptr_t)workspace & 7) == 0 && workspace_bytes >= need,
               "%s: workspace missing, not 8-byte aligned or too small (%zu bytes, %zu needed)", op, workspace_bytes, need);
  hipStream_t s = (hipStream_t)stream;
  FcPartial* partials = (FcPartial*)workspace;
  if (tiles > 0) {
    rc = fc_targets(op, gt_boxes, gt_classes, gt_offsets, G, matched_out, gt_labels, matched_boxes, g, &given);
    if (rc) return rc;
    rc = fc_pointers(op, dtype, logits, deltas, ctrness, anchors, nullptr, nullptr, nullptr, false, P, &vec);
    if (rc) return rc;
    rc = D2_DISPATCH_DTYPE(dtype, [&]() -> int {
      if (given)
        FC_LAUNCH_G(d2amd_fcos_loss_forward_kernel, FC_SRC_GIVEN, gamma, dim3((unsigned)tiles), s, P, p, g, (int)vec,
                    partials);
      else
        FC_LAUNCH_G(d2amd_fcos_loss_forward_kernel, FC_SRC_MATCH, gamma, dim3((unsigned)tiles), s, P, p, g, (int)vec,
                    partials);
      D2_LAUNCH_OK();
      return D2AMD_OK;
    });
    if (rc) return rc;
  }
  hipLaunchKernelGGL(d2amd_fcos_loss_final_kernel, dim3(1), dim3(256), 0, s, partials, (int)tiles, (long)N * R,
                     loss_cls_sum, loss_loc_sum, loss_ctr_sum, stats);
  D2_LAUNCH_OK();
  return D2AMD_OK;
}

extern "C" int d2amd_fcos_loss_backward(const void* const* logits, const void* const* deltas, const void* const* ctrness,
                                        const float* const* anchors, const float* gt_boxes, const int64_t* gt_classes,
                                        const int* gt_offsets, int G, const int* matched, const int64_t* gt_labels,
                                        const float* matched_boxes, const float* grad_cls, const float* grad_loc,
                                        const float* grad_ctr, int N, const int* level_anchors, int L, int K, int dtype,
                                        int normalize_by_size, float alpha, float gamma, void* const* grad_logits,
                                        void* const* grad_deltas, void* const* grad_ctrness, void* stream) {
  const char* op = "fcos_loss_backward";
  FcLevels P; FcParams p{}; FcTargets g{}; int R; long tiles; bool given, vec;
  int rc = fc_layout(op, N, level_anchors, L, K, P, &R, &tiles);
  if (rc) return rc;
  rc = fc_params(op, N, K, R, G, 0.f, normalize_by_size, alpha, gamma, p);
  if (rc) return rc;
  if (tiles == 0) return D2AMD_OK;
  D2_CHECK_ARG(grad_cls && grad_loc && grad_ctr, "%s: null upstream gradient", op);
  rc = fc_targets(op, gt_boxes, gt_classes, gt_offsets, G, const_cast<int*>(matched), gt_labels, matched_boxes, g, &given);
  if (rc) return rc;
  rc = fc_pointers(op, dtype, logits, deltas, ctrness, anchors, grad_logits, grad_deltas, grad_ctrness, true, P, &vec);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  return D2_DISPATCH_DTYPE(dtype, [&]() -> int {
    if (given)
      FC_LAUNCH_G(d2amd_fcos_loss_backward_kernel, FC_SRC_GIVEN, gamma, dim3((unsigned)tiles), s, P, p, g, grad_cls,
                  grad_loc, grad_ctr, (int)vec);
    else
      FC_LAUNCH_G(d2amd_fcos_loss_backward_kernel, FC_SRC_INDEX, gamma, dim3((unsigned)tiles), s, P, p, g, grad_cls,
                  grad_loc, grad_ctr, (int)vec);
    D2_LAUNCH_OK();
    return D2AMD_OK;
  });
}
