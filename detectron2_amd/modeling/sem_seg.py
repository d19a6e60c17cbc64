"""Semantic-segmentation head glue of `detectron2.modeling.meta_arch.semantic_seg` on the hot path, backed by
csrc/sem_seg.hip:

* `sem_seg_loss`: `SemSegFPNHead.losses` (semantic_seg.py:255-267) -- the x `common_stride` bilinear upsampling and the
  cross-entropy in two forward launches (the tile kernel and a one-workgroup sum of its records) and one backward
  launch.  The upsampled logits live in registers: the only full-res buffer is the per-pixel logsumexp (4 B per pixel)
  the backward reads; the gradient is written once, in the dtype and memory format of the logits.
* `sem_seg_labels`: the inference path -- the same upsampling (semantic_seg.py:241-243), `sem_seg_postprocess`
  (postprocessing.py:77-100) and the caller's `argmax(dim=0)` -- as one launch that writes the label map only.

Neither reads anything on the host.
"""
import ctypes
from typing import List, Sequence, Tuple, Union

import torch

from .. import _C

__all__ = ["sem_seg_loss", "sem_seg_loss_with_stats", "sem_seg_labels"]

MAX_CLASSES = 256
SCALES = (2, 4, 8)


def _check_supported(op, predictions, common_stride):
    assert predictions.dim() == 4, f"{op}: predictions must be (N, C, h, w), got {tuple(predictions.shape)}"
    if common_stride not in SCALES:
        raise NotImplementedError(f"{op}: common_stride {common_stride} is not implemented (2, 4 and 8 are)")
    if predictions.shape[1] > MAX_CLASSES:
        raise NotImplementedError(f"{op}: {predictions.shape[1]} classes are not implemented (up to {MAX_CLASSES} are)")


def _dense(x):
    """-> (x or a dense copy, layout code): NCHW-contiguous and channels_last tensors are taken as they are."""
    if x.is_contiguous():
        return x, _C.NCHW
    if x.is_contiguous(memory_format=torch.channels_last):
        return x, _C.NHWC
    return x.contiguous(), _C.NCHW


class _SemSegLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, targets, scale, ignore_value):
        x, layout = _dense(logits)
        n, c, h, w = x.shape
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        stats = torch.empty(2, dtype=torch.int64, device=x.device)
        L = _C.lib()
        ws_bytes = L.d2amd_sem_seg_loss_workspace_bytes(n, h, w, scale)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
        with _C.on_device(x.device):
            _C.check(L.d2amd_sem_seg_loss_forward(_C.ptr(x), _C.ptr(targets), n, c, h, w, scale, _C.dtype_code(x), layout,
                                                  ignore_value, _C.ptr(loss), _C.ptr(stats), _C.ptr(ws),
                                                  ctypes.c_size_t(ws_bytes), _C.stream()))
        # the count and every pixel's logsumexp stay on the device, in `ws`
        ctx.save_for_backward(x, targets, ws)
        ctx.args = (scale, ignore_value, layout)
        ctx.mark_non_differentiable(stats)
        ctx.set_materialize_grads(False)
        return loss, stats

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss, _grad_stats):
        if grad_loss is None:
            return None, None, None, None
        x, targets, ws = ctx.saved_tensors
        scale, ignore_value, layout = ctx.args
        n, c, h, w = x.shape
        g = grad_loss.detach().to(dtype=torch.float32).contiguous()
        grad = torch.empty_like(x)  # (the strides of x: the same layout code)
        with _C.on_device(x.device):
            _C.check(_C.lib().d2amd_sem_seg_loss_backward(_C.ptr(x), _C.ptr(targets), _C.ptr(ws), _C.ptr(g), n, c, h, w,
                                                          scale, _C.dtype_code(x), layout, ignore_value, _C.ptr(grad),
                                                          _C.stream()))
        return grad, None, None, None


def sem_seg_loss_with_stats(predictions: torch.Tensor, targets: torch.Tensor, *, common_stride: int,
                            ignore_value: int = -1, loss_weight: float = 1.0):
    """`sem_seg_loss` and stats int64 [2] on the device: (pixels that count, pixels whose target is neither
    `ignore_value` nor a class -- torch device-asserts on those; here they are ignored and counted)."""
    _C.require_gpu(predictions, targets, op="sem_seg_loss")
    _check_supported("sem_seg_loss", predictions, common_stride)
    n, _, h, w = predictions.shape
    assert n > 0, "sem_seg_loss: empty batch"
    assert tuple(targets.shape) == (n, common_stride * h, common_stride * w), \
        f"sem_seg_loss: targets {tuple(targets.shape)} for predictions {tuple(predictions.shape)} x {common_stride}"
    t = targets.detach()
    if t.dtype != torch.int64:
        t = t.long()
    loss, stats = _SemSegLoss.apply(predictions, t.contiguous(), int(common_stride), int(ignore_value))
    return (loss if loss_weight == 1.0 else loss * loss_weight), stats


def sem_seg_loss(predictions: torch.Tensor, targets: torch.Tensor, *, common_stride: int, ignore_value: int = -1,
                 loss_weight: float = 1.0) -> torch.Tensor:
    """SemSegFPNHead.losses' value: (N, C, h, w) logits (fp32 / f16 / bf16, NCHW or channels_last) and (N, s h, s w)
    integer targets -> the fp32 scalar cross_entropy(interpolate(predictions.float(), scale_factor=s, bilinear,
    align_corners=False), targets, reduction="mean", ignore_index=ignore_value) * loss_weight.  No pixel counts -> NaN,
    as torch's.  s outside {2, 4, 8} or more than 256 classes raise NotImplementedError."""
    return sem_seg_loss_with_stats(predictions, targets, common_stride=common_stride, ignore_value=ignore_value,
                                   loss_weight=loss_weight)[0]


def _labels(x, layout, image_size, output_size, scale):
    n, c, h, w = x.shape
    (ih, iw), (oh, ow) = image_size, output_size
    assert 0 < ih <= scale * h and 0 < iw <= scale * w, (image_size, tuple(x.shape), scale)
    out = torch.empty((n, oh, ow), dtype=torch.int64, device=x.device)
    with _C.on_device(x.device):
        rc = _C.lib().d2amd_sem_seg_labels(_C.ptr(x), n, c, h, w, scale, _C.dtype_code(x), layout, ih, iw, oh, ow,
                                           _C.ptr(out), _C.stream())
    # any unsupported configuration; from Python only the refusal of a downscale whose footprint of one class exceeds
    # the LDS reaches here (scale, classes, layout and dtype are rejected above), and it is made before any launch
    if rc == _C.EUNSUPPORTED:
        raise NotImplementedError(_C.lib().d2amd_last_error().decode())
    _C.check(rc)
    return out


def sem_seg_labels(predictions: torch.Tensor, image_sizes: Sequence[Tuple[int, int]],
                   output_sizes: Sequence[Tuple[int, int]], *, common_stride: int) -> Union[torch.Tensor, List[torch.Tensor]]:
    """Label maps of a batch: for image i, argmax(dim=0) of sem_seg_postprocess(interpolate(predictions, scale_factor=s,
    bilinear, align_corners=False)[i], image_sizes[i], *output_sizes[i]) -- (N, C, h, w) stride-s logits, image_sizes the
    (height, width) of every image inside the padded batch, output_sizes the sizes wanted.  -> a list of (oh, ow) int64
    maps, or ONE (N, oh, ow) tensor from one launch when all images share both sizes.  A downscale so heavy that the
    low-res footprint of 16 x 16 output pixels of ONE class exceeds the LDS raises NotImplementedError."""
    _C.require_gpu(predictions, op="sem_seg_labels")
    _check_supported("sem_seg_labels", predictions, common_stride)
    n = predictions.shape[0]
    sizes = [(tuple(int(v) for v in a), tuple(int(v) for v in b)) for a, b in zip(image_sizes, output_sizes)]
    assert len(sizes) == n and len(image_sizes) == len(output_sizes), (len(image_sizes), len(output_sizes), n)
    x, layout = _dense(predictions.detach())
    if n > 0 and all(s == sizes[0] for s in sizes):
        return _labels(x, layout, *sizes[0], int(common_stride))
    return [_labels(x[i:i + 1], layout, *sizes[i], int(common_stride))[0] for i in range(n)]
