"""GPU parity of the fused semantic-segmentation head (detectron2_amd/csrc/sem_seg.hip) through the public interface,
against plain torch in float64 on the CPU: F.interpolate + F.cross_entropy + autograd for the loss, the two
F.interpolate of the inference path for the labels.
Bars: loss 1e-5 relative.  Gradient, on g * count (a unit-scale quantity): 1e-5 max|g64 * count| -- torch's own fp32
path is within 3.5e-7 of float64 by this measure at these shapes, a wrong tap or phase is O(1) -- plus, for 16-bit I/O,
one rounding of the element (bf16 2^-8, f16 2^-11 relative; f16 subnormals: half their spacing, 2^-25); the reference is
computed on the rounded inputs.  Counts, zeros and run-to-run bits exact.  Labels: at EVERY output pixel the float64
logit of the returned class is within 1e-4 max|logit| of the pixel's maximum."""
import pytest
import torch
import torch.nn.functional as F

from detectron2_amd.modeling import sem_seg_labels, sem_seg_loss, sem_seg_loss_with_stats

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
# (N, C, h, w, s): one low-res pixel (every tap clamped); smaller than a tile; one and two pixels past the forward's
# 16-block tile (two and three past the backward's 15 pixels); class-chunked slabs, C not a multiple; the largest C
LOSS_CASES = [(1, 3, 1, 1, 8), (2, 54, 3, 5, 4), (1, 19, 17, 18, 4), (2, 150, 5, 4, 2), (1, 256, 2, 3, 4)]


def _loss_inputs(case, dtype, channels_last, ignore_value, seed=0):
    N, C, h, w, s = case
    g = torch.Generator().manual_seed(1000 * C + 10 * h + s + seed)
    x = (3 * torch.randn(N, C, h, w, generator=g)).to(dtype)
    t = torch.randint(0, C, (N, s * h, s * w), generator=g)
    t[torch.rand(t.shape, generator=g) < 0.2] = ignore_value
    xd = x.to(DEV)
    if channels_last:
        xd = xd.contiguous(memory_format=torch.channels_last)
    return x, t, xd.requires_grad_(True)


def _reference(x, t, s, ignore_value):
    x64 = x.double().requires_grad_(True)
    up = F.interpolate(x64, scale_factor=s, mode="bilinear", align_corners=False)
    loss = F.cross_entropy(up, t, reduction="mean", ignore_index=ignore_value)
    loss.backward()
    return loss.detach(), x64.grad


def _check_loss(case, dtype, channels_last, ignore_value):
    x, t, xd = _loss_inputs(case, dtype, channels_last, ignore_value)
    ref, g64 = _reference(x, t, case[4], ignore_value)
    loss, stats = sem_seg_loss_with_stats(xd, t.to(DEV), common_stride=case[4], ignore_value=ignore_value)
    (grad,) = torch.autograd.grad(loss, xd)
    count = int((t != ignore_value).sum())
    assert stats.tolist() == [count, 0] and loss.dtype == torch.float32
    assert grad.dtype == dtype and grad.stride() == xd.stride()
    err = (grad.cpu().double() - g64).abs() * count
    tol = 1e-5 * float(g64.abs().max()) * count + EPS[dtype] * g64.abs() * count
    if dtype == torch.float16:
        tol = tol + 2.0 ** -25 * count
    print(f"loss {float(loss.detach()):.7f} ref {float(ref):.7f}; grad err * count {float(err.max()):.3g} "
          f"(1e-5 max = {1e-5 * float(g64.abs().max()) * count:.3g})")
    assert abs(float(loss.detach()) - float(ref)) <= 1e-5 * abs(float(ref))
    assert (err <= tol).all(), float((err - tol).max())
    loss2 = sem_seg_loss(xd, t.to(DEV), common_stride=case[4], ignore_value=ignore_value)
    assert torch.equal(torch.autograd.grad(loss2, xd)[0], grad) and torch.equal(loss2, loss)


@pytest.mark.parametrize("ignore_value", [255, -1])
@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", LOSS_CASES, ids=lambda c: "x".join(map(str, c)))
def test_loss_and_gradient_against_float64(case, dtype, channels_last, ignore_value):
    _check_loss(case, dtype, channels_last, ignore_value)


def test_loss_and_gradient_f16():
    _check_loss(LOSS_CASES[1], torch.float16, False, 255)


def test_ignored_regions():
    case, s, ign = (2, 7, 6, 5, 4), 4, 255
    x, t, xd = _loss_inputs(case, torch.float32, False, ign)
    # one image entirely ignored: no gradient there, the loss of the other image alone
    t1 = t.clone()
    t1[1] = ign
    loss, stats = sem_seg_loss_with_stats(xd, t1.to(DEV), common_stride=s, ignore_value=ign)
    (grad,) = torch.autograd.grad(loss, xd)
    ref, g64 = _reference(x[:1], t1[:1], s, ign)
    assert (grad[1] == 0).all() and int(stats[0]) == int((t1 != ign).sum())
    assert abs(float(loss) - float(ref)) <= 1e-5 * abs(float(ref))
    assert ((grad[0].cpu().double() - g64[0]).abs() <= 1e-5 * g64.abs().max()).all()
    # out-of-range targets: counted in stats[1], otherwise as if ignored
    t2 = t.clone()
    bad = torch.rand(t.shape, generator=torch.Generator().manual_seed(3)) < 0.1
    t2[bad] = torch.where(torch.arange(int(bad.sum())) % 2 == 0, 7 + 3, -7)
    t2_ign = torch.where(bad, ign, t)
    loss, stats = sem_seg_loss_with_stats(xd, t2.to(DEV), common_stride=s, ignore_value=ign)
    (grad,) = torch.autograd.grad(loss, xd)
    ref, g64 = _reference(x, t2_ign, s, ign)
    assert stats.tolist() == [int((t2_ign != ign).sum()), int(bad.sum())]
    assert abs(float(loss) - float(ref)) <= 1e-5 * abs(float(ref))
    assert ((grad.cpu().double() - g64).abs() <= 1e-5 * g64.abs().max()).all()
    # nothing counts: NaN as torch's mean over no element, count 0
    loss, stats = sem_seg_loss_with_stats(xd, torch.full_like(t, ign).to(DEV), common_stride=s, ignore_value=ign)
    assert torch.isnan(loss) and stats.tolist() == [0, 0]


# (C, h, w, s, (ih, iw), (oh, ow)): identity; the padding cropped + an upscale over several tiles; a non-integer
# downscale; one low-res pixel
LABEL_CASES = [(5, 6, 7, 4, (24, 28), (24, 28)), (54, 9, 11, 4, (33, 41), (50, 61)), (19, 20, 23, 2, (37, 45), (15, 18)),
               (3, 1, 1, 8, (8, 8), (5, 9))]


@pytest.mark.parametrize("dtype,channels_last", [(torch.float32, False), (torch.bfloat16, True)], ids=["fp32-nchw", "bf16-nhwc"])
@pytest.mark.parametrize("case", LABEL_CASES, ids=lambda c: "x".join(map(str, c[:4])))
def test_labels_against_float64(case, dtype, channels_last):
    C, h, w, s, (ih, iw), (oh, ow) = case
    x = (3 * torch.randn(2, C, h, w, generator=torch.Generator().manual_seed(C + h))).to(dtype)
    xd = x.to(DEV)
    if channels_last:
        xd = xd.contiguous(memory_format=torch.channels_last)
    labels = sem_seg_labels(xd, [(ih, iw)] * 2, [(oh, ow)] * 2, common_stride=s)
    assert labels.shape == (2, oh, ow) and labels.dtype == torch.int64
    up = F.interpolate(x.double(), scale_factor=s, mode="bilinear", align_corners=False)
    ref = F.interpolate(up[:, :, :ih, :iw], size=(oh, ow), mode="bilinear", align_corners=False)
    got = labels.cpu()
    assert (got >= 0).all() and (got < C).all()
    short = ref.max(dim=1).values - ref.gather(1, got[:, None])[:, 0]
    print(f"labels: {int((got != ref.argmax(dim=1)).sum())} of {got.numel()} differ from float64's argmax, worst "
          f"shortfall {float(short.max()):.3g} (bar {1e-4 * float(x.double().abs().max()):.3g})")
    assert (short <= 1e-4 * float(x.double().abs().max())).all()
    # images of different sizes: a list, one launch each
    per_image = sem_seg_labels(xd, [(ih, iw), (ih, iw)], [(oh, ow), (oh + 1, ow)], common_stride=s)
    assert torch.equal(per_image[0], labels[0]) and per_image[1].shape == (oh + 1, ow)
    zeros = sem_seg_labels(torch.zeros_like(xd), [(ih, iw)] * 2, [(oh, ow)] * 2, common_stride=s)
    assert (zeros == 0).all()


def test_rejections():
    x = torch.zeros(1, 4, 3, 3, device=DEV)
    with pytest.raises(NotImplementedError):
        sem_seg_loss(x, torch.zeros(1, 9, 9, dtype=torch.int64, device=DEV), common_stride=3)
    with pytest.raises(NotImplementedError):
        sem_seg_labels(x, [(9, 9)], [(9, 9)], common_stride=3)
    with pytest.raises(NotImplementedError):
        sem_seg_loss(torch.zeros(1, 257, 3, 3, device=DEV), torch.zeros(1, 12, 12, dtype=torch.int64, device=DEV),
                     common_stride=4)
    with pytest.raises(AssertionError):
        sem_seg_loss(x, torch.zeros(1, 12, 11, dtype=torch.int64, device=DEV), common_stride=4)
