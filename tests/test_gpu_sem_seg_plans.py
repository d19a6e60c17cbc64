"""The fused semantic-segmentation head (detectron2_amd/csrc/sem_seg.hip) on every tile plan of its host code, at tile
edges, with a looping final reduction, at a large logit spread, with class-chunked label decodes and at the host's
footprint bound -- the parts of the plan space tests/test_gpu_sem_seg.py does not reach.  Same interface, same float64
CPU references (F.interpolate + F.cross_entropy + autograd; the two F.interpolate of the inference path) and the same
bars as that file:
  loss 1e-5 relative; gradient, on g * count, 1e-5 max|g64 * count| plus one rounding of a 16-bit element; counts,
  zeros and run-to-run bits exact; labels: the float64 logit of the returned class within 1e-4 max|logit| of the
  pixel's maximum, at every pixel.
The bars at the logit spread of SPREAD_KINDS were checked before use, without the kernel: the same formulas in fp32
torch on the CPU (interpolate, cross_entropy, autograd) against float64 on exactly these inputs differ by
  spikes 2x5x17x19x8: loss 5.5e-8 relative, gradient 3.6e-7 max|g64|;  2x7x16x15x4: 1.2e-7, 2.7e-7
  plane  2x5x17x19x8: loss 1.2e-8 relative, gradient 6.5e-7 max|g64|;  2x7x16x15x4: 1.6e-8, 3.7e-7
  f16    2x5x17x19x8: loss 4.8e-9 relative, gradient 3.3e-7 max|g64|;  2x7x16x15x4: 7.0e-8, 1.7e-7
(3 randn alone on the same shapes: 1.9e-8, 4.8e-7 and 5.6e-8, 2.7e-7) -- all under a quarter of the bars (2.5e-6), so
the bars stay as they are.  No number here comes from the kernel."""
import functools

import pytest
import torch
import torch.nn.functional as F

from detectron2_amd.modeling import sem_seg_labels, sem_seg_loss, sem_seg_loss_with_stats
from test_gpu_sem_seg import DEV, EPS, _reference

gpu = pytest.mark.gpu  # on every test but the pure-Python check of the case table, which the CPU suite runs too

# (N, C, h, w, s), one row per reachable (scale group, direction, tuy, LDS budget) of ss_plan, C on the band edges, the
# smallest h, w (give or take one) at which forward AND backward launch >= 2 x 2 tiles.  test_plan_table_covers_every_plan
# checks the comments against _plan.
PLAN_CASES = [
    # scale 2 and 4 (one 16 x tuy tile of whole blocks)
    (2, 55, 16, 16, 4),   # forward 16 (80K), backward 16 (80K)
    (1, 56, 16, 17, 2),   # forward 16 (80K), backward  8 (80K)
    (1, 69, 16, 16, 2),   # forward 16 (80K), backward  8 (80K)
    (1, 70, 8, 16, 4),    # forward  8 (80K), backward  8 (80K)
    (1, 118, 8, 17, 2),   # forward  8 (80K), backward  8 (80K)
    (1, 119, 8, 16, 2),   # forward  8 (80K), backward  4 (80K)
    (1, 132, 9, 16, 4),   # forward  8 (80K), backward  4 (80K)
    (1, 133, 4, 16, 2),   # forward  4 (80K), backward  4 (80K)
    (2, 225, 5, 17, 4),   # forward  4 (80K), backward  4 (80K)
    (1, 226, 8, 16, 2),   # forward  4 (80K), backward  8 (160K)
    (1, 237, 8, 16, 4),   # forward  4 (80K), backward  8 (160K)
    (1, 238, 8, 16, 2),   # forward  8 (160K), backward 8 (160K)
    (1, 252, 8, 17, 4),   # forward  8 (160K), backward 8 (160K)
    (1, 253, 8, 16, 2),   # forward  8 (160K), backward 4 (160K)
    (1, 256, 9, 16, 4),   # forward  8 (160K), backward 4 (160K)
    # scale 8 (four threads per block, 8 blocks per tile row)
    (1, 199, 8, 8, 8),    # forward 16 (80K), backward 16 (80K)
    (1, 200, 8, 9, 8),    # forward 16 (80K), backward  8 (80K)
    (1, 249, 8, 8, 8),    # forward 16 (80K), backward  8 (80K)
    (1, 250, 4, 8, 8),    # forward  8 (80K), backward  8 (80K)
    (1, 256, 5, 9, 8),    # forward  8 (80K), backward  8 (80K)
]
# exactly one full tile / a second tile that holds nothing but the border block, in y and in x, forward (w + 1 blocks in
# steps of 16, scale 8: of 8) and backward (w pixels in steps of 15, scale 8: of 7) at once
EDGE_CASES = [(2, 3, 15, 16, 4), (2, 3, 16, 15, 4), (2, 3, 15, 16, 2), (2, 3, 16, 15, 2), (2, 3, 7, 8, 8), (2, 3, 8, 7, 8)]
MANY_TILES_S8 = (2, 5, 17, 19, 8)  # scale 8 over 3 x 3 tiles, few classes
FINAL_LOOP = (30, 2, 16, 16, 8)    # 3 x 3 x 30 = 270 forward workgroups: the final reduction's stride loop runs twice
LOSS_CASES = PLAN_CASES + EDGE_CASES + [MANY_TILES_S8, FINAL_LOOP]
# bf16 and channels_last: a row of each scale group, three dynamic-LDS sizes above 64 KB ((1, 238, ...): 142 KB forward,
# 154 KB backward), an edge row
SUBSET = [(1, 56, 16, 17, 2), (1, 238, 8, 16, 2), (1, 250, 4, 8, 8), (2, 3, 16, 15, 4), MANY_TILES_S8]
SPREAD_CASES = [MANY_TILES_S8, (2, 7, 16, 15, 4)]
SPREAD_KINDS = ["spikes", "plane", "f16"]
_ids = lambda c: "x".join(map(str, c))


def _plan(C, h, w, s, backward):
    """-> (tuy, LDS budget, tiles_x, tiles_y): a restatement of ss_plan, detectron2_amd/csrc/sem_seg.hip:439-455, and
    of its constants at :46-51.  It must change with them.  Used ONLY to check that the case table covers every plan."""
    q = s // min(s, 4)
    for budget in (80 * 1024, 160 * 1024):
        for tuy in (16, 8, 4):
            bxn, byn = 16 // q, tuy // q
            lds = C * (bxn + 1) * (byn + 1) * 4 + (2 * 2 * 16 * tuy * 16 if backward else 0)
            if lds + 1024 <= budget:
                tiles = (-(-w // (bxn - 1)), -(-h // (byn - 1))) if backward else (-(-(w + 1) // bxn), -(-(h + 1) // byn))
                return (tuy, budget) + tiles
    raise AssertionError("no plan")


def test_plan_table_covers_every_plan():
    reachable = {(s == 8, bwd) + _plan(C, 1, 1, s, bwd)[:2] for s in (2, 4, 8) for bwd in (False, True)
                 for C in range(1, 257)}
    assert len(reachable) == 4 + 5 + 2 + 2, sorted(reachable)
    covered = set()
    for N, C, h, w, s in PLAN_CASES:
        for bwd in (False, True):
            tuy, budget, tx, ty = _plan(C, h, w, s, bwd)
            assert tx >= 2 and ty >= 2, ((N, C, h, w, s), bwd, tuy, tx, ty)
            covered.add((s == 8, bwd, tuy, budget))
    assert covered == reachable, sorted(reachable - covered)
    for case in EDGE_CASES + [MANY_TILES_S8]:
        assert all(_plan(*case[1:], bwd)[2] * _plan(*case[1:], bwd)[3] >= 2 for bwd in (False, True)), case
    N, C, h, w, s = FINAL_LOOP
    assert N * _plan(C, h, w, s, False)[2] * _plan(C, h, w, s, False)[3] > 256


@functools.lru_cache(maxsize=None)
def _inputs(case, dtype, ignore_value, kind="randn"):
    """-> x (CPU, rounded to dtype), targets with ~20 % ignored, ~5 % out of range (above C - 1 and negative) and an
    ignored corner, the targets with the out-of-range ones ignored, and the float64 reference (loss, gradient) on those.
    Computed once per (case, dtype, ignore_value, kind) and shared: nobody writes into what this returns."""
    N, C, h, w, s = case
    g = torch.Generator().manual_seed(1000 * C + 10 * h + s + 77)
    x = 3 * torch.randn(N, C, h, w, generator=g)
    if kind in ("spikes", "f16"):  # six elements per image at +-60
        for n in range(N):
            x[n].view(-1)[torch.randint(0, C * h * w, (6,), generator=g)] = torch.tensor([60.0, -60.0] * 3)
    if kind == "plane":  # one class + 60 everywhere, the others - 60: a pixel's loss is 0 (target C // 2) or 120
        x[:] = -60.0
        x[:, C // 2] = 60.0
    big = [(0, 1, h // 2, w // 2), (0, 2, h // 2 + 2, 2)] if kind == "f16" else []
    for at, v in zip(big, (6e4, -6e4)):  # saturation of f16, in different classes (inside one class the two would cancel
        x[at] = v                         # to O(1) values known to 6e4 * 2^-24 only), both away from the ignored corner
    x = x.to(dtype)
    t = torch.randint(0, C, (N, s * h, s * w), generator=g)
    u = torch.rand(t.shape, generator=g)
    t[u < 0.2] = ignore_value
    bad = (u >= 0.2) & (u < 0.25)
    t[bad] = torch.where(torch.arange(int(bad.sum())) % 2 == 0, C + 300, -7)
    # every full-res pixel that reaches the low-res pixels (0..1, w - 2..w - 1) is ignored: their gradient is exactly 0
    t[:, :3 * s, s * (w - 3):] = ignore_value
    bad[:, :3 * s, s * (w - 3):] = False
    t_ign = torch.where(bad, ignore_value, t)
    ref = _reference(x, t_ign, s, ignore_value)
    assert all(ref[1][at] != 0 for at in big)  # counted pixels interpolate both saturated elements
    return x, t, t_ign, ref


def _check_loss(case, dtype, channels_last, ignore_value, kind="randn"):
    s = case[4]
    x, t, t_ign, (ref, g64) = _inputs(case, dtype, ignore_value, kind)
    xd = x.to(DEV)
    if channels_last:
        xd = xd.contiguous(memory_format=torch.channels_last)
    xd.requires_grad_(True)
    loss, stats = sem_seg_loss_with_stats(xd, t.to(DEV), common_stride=s, ignore_value=ignore_value)
    (grad,) = torch.autograd.grad(loss, xd)
    count, oob = int((t_ign != ignore_value).sum()), int((t != t_ign).sum())
    assert oob > 0 and stats.tolist() == [count, oob] and loss.dtype == torch.float32
    assert grad.dtype == dtype and grad.stride() == xd.stride()
    err = (grad.cpu().double() - g64).abs() * count
    tol = 1e-5 * float(g64.abs().max()) * count + EPS[dtype] * g64.abs() * count
    if dtype == torch.float16:
        tol = tol + 2.0 ** -25 * count
    print(f"loss {float(loss.detach()):.7f} ref {float(ref):.7f}; grad err * count {float(err.max()):.3g} "
          f"(1e-5 max = {1e-5 * float(g64.abs().max()) * count:.3g})")
    assert abs(float(loss.detach()) - float(ref)) <= 1e-5 * abs(float(ref))
    assert (err <= tol).all(), float((err - tol).max())
    zero = (g64 == 0).all(dim=1, keepdim=True).expand_as(g64)
    assert zero[:, :, :2, -2:].all() and (grad.cpu()[zero] == 0).all()
    loss2 = sem_seg_loss(xd, t.to(DEV), common_stride=s, ignore_value=ignore_value)
    assert torch.equal(torch.autograd.grad(loss2, xd)[0], grad) and torch.equal(loss2, loss)


@gpu
@pytest.mark.parametrize("case", LOSS_CASES, ids=_ids)
def test_loss_and_gradient_on_every_plan(case):
    _check_loss(case, torch.float32, False, 255)


@gpu
@pytest.mark.parametrize("dtype,channels_last", [(torch.bfloat16, False), (torch.float32, True), (torch.bfloat16, True)],
                         ids=["bf16-nchw", "fp32-nhwc", "bf16-nhwc"])
@pytest.mark.parametrize("case", SUBSET, ids=_ids)
def test_loss_and_gradient_bf16_and_channels_last(case, dtype, channels_last):
    _check_loss(case, dtype, channels_last, -1)


@gpu
@pytest.mark.parametrize("case", [MANY_TILES_S8, (1, 56, 16, 17, 2)], ids=_ids)
def test_loss_and_gradient_f16(case):
    _check_loss(case, torch.float16, False, 255)


@gpu
@pytest.mark.parametrize("kind", SPREAD_KINDS)
@pytest.mark.parametrize("case", SPREAD_CASES, ids=_ids)
def test_logit_spread(case, kind):
    _check_loss(case, torch.float16 if kind == "f16" else torch.float32, False, 255, kind)


# ---- label decode -----------------------------------------------------------------------------------------------------
def _labels_reference(x, s, image_size, output_size):
    up = F.interpolate(x.double(), scale_factor=s, mode="bilinear", align_corners=False)
    return F.interpolate(up[:, :, :image_size[0], :image_size[1]], size=output_size, mode="bilinear", align_corners=False)


def _check_labels(x, xd, s, image_size, output_size):
    N, C = x.shape[:2]
    labels = sem_seg_labels(xd, [image_size] * N, [output_size] * N, common_stride=s)
    assert labels.shape == (N,) + tuple(output_size) and labels.dtype == torch.int64
    ref = _labels_reference(x, s, image_size, output_size)
    got = labels.cpu()
    assert (got >= 0).all() and (got < C).all()
    short = ref.max(dim=1).values - ref.gather(1, got[:, None])[:, 0]
    print(f"labels: {int((got != ref.argmax(dim=1)).sum())} of {got.numel()} differ from float64's argmax, worst "
          f"shortfall {float(short.max()):.3g} (bar {1e-4 * float(x.double().abs().max()):.3g})")
    assert (short <= 1e-4 * float(x.double().abs().max())).all()


# (C, h, w, s, (ih, iw), (oh, ow)).  The kernel stages min(C, 16384 / P) classes at a time, P the low-res footprint of a
# 16 x 16 output tile, once C fh fw 4 > 64 KB (fh, fw: the host's bound on the footprint's sides, which caps the LDS).
# CHUNK_CASES loop over class chunks in the kernel:
#   256 x 9 x 9, scale 4, (36, 36) -> (16, 16): one tile over all 81 pixels, chunks of 202 -> 2;
#   200 x 12 x 11, scale 2: identity size, a 10 x 10 footprint, chunks of 163 -> 2; (24, 22) -> (16, 15): all 132 pixels,
#     chunks of 124 -> 2;
#   256 x 12 x 12, scale 2, (24, 24) -> (16, 16): one tile over all 144 pixels, chunks of 113 -> 3.
CHUNK_CASES = [(256, 9, 9, 4, (36, 36), (16, 16)), (200, 12, 11, 2, (24, 22), (24, 22)), (200, 12, 11, 2, (24, 22), (16, 15)),
               (256, 12, 12, 2, (24, 24), (16, 16))]
# CAPPED_LDS_CASES get the LDS capped at 64 KB by the host's bound (83 KB, 106 KB), but every tile's real footprint is
# small enough for all classes at once: at the identity size of scale 4 a tile's 16 rows span 5 blocks, 6 x 6 pixels,
# and an upscale needs fewer.  No chunk loop here: the one pass must cope with an LDS smaller than C fh fw.
CAPPED_LDS_CASES = [(256, 9, 9, 4, (36, 36), (36, 36)), (256, 9, 9, 4, (34, 35), (50, 61)), (200, 12, 11, 2, (23, 21), (31, 40))]
_label_ids = lambda c: "x".join(map(str, c[:4] + c[5]))


def _check_random_labels(case):
    C, h, w, s, image_size, output_size = case
    x = 3 * torch.randn(2, C, h, w, generator=torch.Generator().manual_seed(C + h))
    _check_labels(x, x.to(DEV), s, image_size, output_size)


@gpu
@pytest.mark.parametrize("case", CHUNK_CASES, ids=_label_ids)
def test_labels_class_chunks(case):
    _check_random_labels(case)


@gpu
@pytest.mark.parametrize("case", CAPPED_LDS_CASES, ids=_label_ids)
def test_labels_capped_lds_all_classes_at_once(case):
    _check_random_labels(case)


@gpu
def test_labels_tie_across_chunks():
    """The same positive map in a class of the first chunk and in one of the last (of three): bit-equal values, and the
    lower class wins at every pixel."""
    C, h, w, s, image_size, output_size = CHUNK_CASES[-1]
    lo, hi = 5, 250  # chunks of 113: classes 0..112, 113..225, 226..255
    x = torch.zeros(2, C, h, w)
    x[:, lo] = x[:, hi] = 0.5 + torch.rand(2, h, w, generator=torch.Generator().manual_seed(5))
    for sizes in [(image_size, output_size), ((24, 24), (24, 24))]:
        labels = sem_seg_labels(x.to(DEV), [sizes[0]] * 2, [sizes[1]] * 2, common_stride=s)
        assert (labels == lo).all(), labels.unique().tolist()


def _axis_grid(s):
    """(h, ih, oh) of the footprint sweep: every image size from the padded one down to half of it, output sizes around
    the 16-pixel tile and downscales of 10 x and more."""
    grid = [(h, ih, oh) for h in (1, 2, 7, 33) for ih in sorted({s * h, s * h - s + 1, -(-s * h // 2)})
            for oh in (1, 3, 16, 17, 33)]
    assert any(ih >= 10 * oh for _, ih, oh in grid) and len(grid) >= 50
    return grid


@gpu
@pytest.mark.parametrize("s", [2, 4, 8])
def test_labels_footprint_bound_one_class(s):
    """C = 1: the kernel's LDS is exactly the host's bound fh * fw on a tile's footprint (sem_seg.hip:562-571), and a tile
    whose footprint is larger answers -1.  Each axis alone (the other axis one pixel, so that its slack cannot hide a
    shortfall), then both at once.  (Restating ss_label_taps in fp32 on the CPU over this grid: where h does not clamp
    the bound, it has two rows to spare -- the test notices a bound that loses three.)"""
    grid = _axis_grid(s)
    one = (1, 1, 1)
    combos = [(a, one) for a in grid] + [(one, a) for a in grid] + [(a, grid[(7 * i + 3) % len(grid)]) for i, a in enumerate(grid)]
    g = torch.Generator().manual_seed(s)
    wrong = []
    for (h, ih, oh), (w, iw, ow) in combos:
        x = torch.randn(1, 1, h, w, generator=g).to(DEV)
        wrong.append((sem_seg_labels(x, [(ih, iw)], [(oh, ow)], common_stride=s) != 0).sum())
    wrong = torch.stack(wrong).cpu().tolist()
    assert not any(wrong), [(c, n) for c, n in zip(combos, wrong) if n]


@gpu
@pytest.mark.parametrize("dtype,channels_last", [(torch.float32, False), (torch.bfloat16, True)], ids=["fp32-nchw", "bf16-nhwc"])
def test_labels_heavy_downscale(dtype, channels_last):
    C, h, w, s = 7, 33, 35, 8
    x = (3 * torch.randn(2, C, h, w, generator=torch.Generator().manual_seed(11))).to(dtype)
    xd = x.to(DEV)
    if channels_last:
        xd = xd.contiguous(memory_format=torch.channels_last)
    _check_labels(x, xd, s, (264, 280), (20, 23))


@gpu
def test_labels_reject_a_footprint_beyond_the_lds():
    # sem_seg.hip:561-570: sy = sx = 800, fh = fw = min(400, floor(800 * 15 / 2) + 6) = 400: 400 * 400 * 4 B = 625 KB of
    # one class do not fit 160 KB -- refused on the host, before any launch
    x = torch.zeros(1, 1, 400, 400, device=DEV)
    with pytest.raises(NotImplementedError):
        sem_seg_labels(x, [(800, 800)], [(1, 1)], common_stride=2)
    assert (sem_seg_labels(x, [(800, 800)], [(40, 40)], common_stride=2) == 0).all()  # 20 x: a 156 x 156 footprint fits


# ---- input forms ------------------------------------------------------------------------------------------------------
@gpu
def test_non_dense_predictions():
    N, C, h, w, s = 2, 5, 6, 17, 4
    g = torch.Generator().manual_seed(9)
    base = (3 * torch.randn(N, C, h, w + 1, generator=g)).to(DEV)
    t = torch.randint(0, C, (N, s * h, s * w), generator=g).to(DEV)
    view = base[:, :, ::1, 1:].requires_grad_(True)
    dense = view.detach().contiguous().requires_grad_(True)
    assert not view.is_contiguous() and not view.is_contiguous(memory_format=torch.channels_last)
    loss_v = sem_seg_loss(view, t, common_stride=s)
    loss_d = sem_seg_loss(dense, t, common_stride=s)
    (grad_v,), (grad_d,) = torch.autograd.grad(loss_v, view), torch.autograd.grad(loss_d, dense)
    assert grad_v.shape == view.shape and bool(grad_d.abs().max() > 0)
    assert torch.equal(loss_v, loss_d) and torch.equal(grad_v, grad_d)


@gpu
@pytest.mark.parametrize("tdtype", [torch.int32, torch.uint8])
def test_target_dtypes(tdtype):
    N, C, h, w, s = 2, 7, 5, 18, 4
    g = torch.Generator().manual_seed(13)
    x = (3 * torch.randn(N, C, h, w, generator=g)).to(DEV)
    t = torch.randint(0, C, (N, s * h, s * w), generator=g)
    u = torch.rand(t.shape, generator=g)
    t[u < 0.2] = 255
    t[u > 0.95] = 200  # out of range in either dtype
    out = []
    for tt in (t, t.to(tdtype)):
        xd = x.clone().requires_grad_(True)
        loss, stats = sem_seg_loss_with_stats(xd, tt.to(DEV), common_stride=s, ignore_value=255)
        out.append((loss.detach(), stats, torch.autograd.grad(loss, xd)[0]))
    assert out[0][1].tolist() == [int(((u >= 0.2) & (u <= 0.95)).sum()), int(((u > 0.95)).sum())]
    assert all(torch.equal(a, b) for a, b in zip(*out))
