"""Training head of FCOS on the hot path (meta_arch/fcos.py:86-251), backed by csrc/fcos.hip:

* `fcos_losses_from_gt` is the fused form: the point matching of `FCOS.label_anchors`, the sigmoid focal loss, GIoU through
  `Box2BoxTransformLinear` and the centerness BCE of all images and levels in one forward and one backward launch.  No
  [N,R] labels, [N,R,4] matched boxes, centerness targets, one-hot or concatenated logits exist; an int32 `matched`
  [N,R] is all the backward keeps.
* `fcos_losses` is `FCOS.losses` with the reference's arguments: the same kernels, the targets read from the given
  `gt_labels` / `gt_boxes`.  `fcos_label_anchors` is `FCOS.label_anchors` for the whole batch.
* Nothing reads the host: the positive count stays on the device (`stats`, which `ema_normalizer_` takes), so a training
  step that uses these losses can be captured into a graph.  Pass the ground truth packed, with its offsets on the
  device, and a captured step replays with other ground-truth counts."""
import ctypes
from typing import List, Sequence, Union

import torch

from .. import _C
from .dense_loss import _ptrs, _stacked, _tensor

__all__ = ["fcos_label_anchors", "fcos_losses", "fcos_losses_from_gt", "FCOS_GT_CHUNK"]

FCOS_GT_CHUNK = 128  # ground-truth boxes staged in LDS at a time (D2AMD_FCOS_GT_CHUNK of include/d2amd.h)


def _anchors(anchors, op):
    an = [_tensor(a) for a in anchors]
    if any(a.shape[-1] != 4 for a in an):
        raise NotImplementedError(f"{op}: 5-column (rotated) anchors are not implemented")
    if any(a.shape[0] == 0 for a in an):  # (the reference's `upper_bound[-0:] = inf` would cover every level)
        raise ValueError(f"{op}: a level without anchor points ({[a.shape[0] for a in an]})")
    return an


def _pack_gt(gt_boxes_list, gt_classes_list, gt_offsets, dev, op):
    """-> (boxes fp32 [G,4], classes int64 [G], offsets int32 [N+1]) on the device.  With `gt_offsets` the two lists are
    already the packed tensors; otherwise the offsets come from the lists' shapes (host knowledge, no device read)."""
    if gt_offsets is not None:
        boxes, classes = _tensor(gt_boxes_list).reshape(-1, 4), gt_classes_list
        _C.require_gpu(boxes, classes, gt_offsets, op=op)
        assert gt_offsets.dtype == torch.int32 and classes.shape[0] == boxes.shape[0], (gt_offsets.dtype, classes.shape)
        return (boxes.detach().to(torch.float32).contiguous(), classes.to(torch.int64).contiguous(),
                gt_offsets.contiguous())
    gts = [_tensor(g).reshape(-1, 4) for g in gt_boxes_list]
    assert len(gts) == len(gt_classes_list), (len(gts), len(gt_classes_list))
    _C.require_gpu(*gts, *gt_classes_list, op=op)
    counts = [int(g.shape[0]) for g in gts]
    assert counts == [int(c.shape[0]) for c in gt_classes_list], (counts, [c.shape for c in gt_classes_list])
    offs = [0]
    for c in counts:
        offs.append(offs[-1] + c)
    offsets = torch.tensor(offs, dtype=torch.int32).pin_memory().to(dev, non_blocking=True)
    if offs[-1] == 0:
        return (torch.zeros((0, 4), dtype=torch.float32, device=dev), torch.zeros(0, dtype=torch.int64, device=dev),
                offsets)
    boxes = torch.cat([g.detach().to(torch.float32) for g in gts]).contiguous()
    classes = torch.cat([c.to(torch.int64) for c in gt_classes_list]).contiguous()
    return boxes, classes, offsets


@torch.no_grad()
def fcos_label_anchors(anchors: Sequence, gt_boxes_list, gt_classes_list, num_classes: int,
                       center_sampling_radius: float = 1.5, return_matched: bool = False, *, gt_offsets=None):
    """`FCOS.label_anchors` (fcos.py:153-191) for the whole batch in one launch, bit-exact against the reference's fp32
    matching.  anchors[l] [A_l,4] (Tensor or Boxes): the points are the anchors' centres, their size the stride;
    gt_boxes_list[i] [M_i,4] and gt_classes_list[i] [M_i] per image, or the packed [G,4] / [G] tensors with
    `gt_offsets` int32 [N+1] on the device.
    -> (gt_labels [N,R] int64: num_classes background, else the matched class; gt_boxes [N,R,4] fp32: the matched box,
    the image's box 0 for an unmatched point, zeros for an image without ground truth), and matched [N,R] int32 (index
    inside the image's ground truth, -1 background) when `return_matched`."""
    op = "fcos_label_anchors"
    an = _anchors(anchors, op)
    _C.require_gpu(*an, op=op)
    n = len(gt_boxes_list) if gt_offsets is None else gt_offsets.numel() - 1
    dev = an[0].device if an else torch.device("cuda")
    r = sum(a.shape[0] for a in an)
    labels = torch.empty((n, r), dtype=torch.int64, device=dev)
    boxes = torch.empty((n, r, 4), dtype=torch.float32, device=dev)
    matched = torch.empty((n, r), dtype=torch.int32, device=dev) if return_matched else None
    if n > 0 and r > 0:
        gb, gc, go = _pack_gt(gt_boxes_list, gt_classes_list, gt_offsets, dev, op)
        an = [a.detach().to(dtype=torch.float32).contiguous() for a in an]
        sizes = (ctypes.c_int * len(an))(*[int(a.shape[0]) for a in an])
        with _C.on_device(dev):
            _C.check(_C.lib().d2amd_fcos_label_anchors(_ptrs(an), _C.ptr(gb), _C.ptr(gc), _C.ptr(go), gb.shape[0], n, sizes,
                                                       len(an), int(num_classes), float(center_sampling_radius),
                                                       _C.ptr(labels), _C.ptr(boxes), _C.ptr(matched), _C.stream()))
    return (labels, boxes, matched) if return_matched else (labels, boxes)


class _FcosLoss(torch.autograd.Function):
    """(cfg, targets, L, *anchors, *logits, *deltas, *centerness) -> (cls_sum, loc_sum, ctr_sum, stats).
    targets: (gt_boxes [G,4], gt_classes [G], gt_offsets [N+1]) packed, or (gt_labels [N,R], gt_boxes [N,R,4]) given."""

    @staticmethod
    def forward(ctx, cfg, targets, nl, *levels):
        anchors = levels[:nl]
        lg, dl, ct = ([t.contiguous() for t in levels[i * nl:(i + 1) * nl]] for i in (1, 2, 3))
        dev = lg[0].device
        n, k = lg[0].shape[0], lg[0].shape[2]
        r = sum(int(a.shape[0]) for a in anchors)
        sizes = (ctypes.c_int * nl)(*[int(a.shape[0]) for a in anchors])
        given = len(targets) == 2
        if given:
            matched = None
            tg = (None, None, None, 0, _C.ptr(targets[0]), _C.ptr(targets[1]))
        else:
            matched = torch.empty((n, r), dtype=torch.int32, device=dev)
            tg = (_C.ptr(targets[0]), _C.ptr(targets[1]), _C.ptr(targets[2]), int(targets[0].shape[0]), None, None)
        out = [torch.empty((), dtype=torch.float32, device=dev) for _ in range(3)]
        stats = torch.empty(2, dtype=torch.int64, device=dev)
        L = _C.lib()
        with _C.on_device(dev):
            ws_bytes = L.d2amd_fcos_loss_workspace_bytes(n, sizes, nl)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            _C.check(L.d2amd_fcos_loss_forward(_ptrs(lg), _ptrs(dl), _ptrs(ct), _ptrs(anchors), *tg, n, sizes, nl, k,
                                               _C.dtype_code(lg[0]), cfg["radius"], cfg["norm"], cfg["alpha"],
                                               cfg["gamma"], _C.ptr(matched), *[_C.ptr(o) for o in out], _C.ptr(stats),
                                               _C.ptr(ws), ctypes.c_size_t(ws_bytes), _C.stream()))
        # nothing per element is kept: the backward recomputes the gradients from the inputs and `matched`
        saved = list(targets) + ([] if given else [matched])
        ctx.save_for_backward(*saved, *anchors, *lg, *dl, *ct)
        ctx.nl, ctx.sizes, ctx.cfg, ctx.nt = nl, sizes, cfg, len(saved)
        ctx.mark_non_differentiable(stats)
        ctx.set_materialize_grads(False)
        return (*out, stats)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_cls, grad_loc, grad_ctr, _grad_stats):
        nl, cfg = ctx.nl, ctx.cfg
        if grad_cls is None and grad_loc is None and grad_ctr is None:
            return (None,) * (3 + 4 * nl)
        tgt, lv = ctx.saved_tensors[:ctx.nt], ctx.saved_tensors[ctx.nt:]
        anchors, lg, dl, ct = (lv[i * nl:(i + 1) * nl] for i in range(4))
        dev = lg[0].device
        up = [torch.zeros((), dtype=torch.float32, device=dev) if g is None else
              g.detach().to(dtype=torch.float32).contiguous() for g in (grad_cls, grad_loc, grad_ctr)]
        grads = [[torch.empty_like(t) for t in ts] for ts in (lg, dl, ct)]
        if ctx.nt == 2:
            tg = (None, None, None, 0, None, _C.ptr(tgt[0]), _C.ptr(tgt[1]))
        else:
            tg = (_C.ptr(tgt[0]), _C.ptr(tgt[1]), _C.ptr(tgt[2]), int(tgt[0].shape[0]), _C.ptr(tgt[3]), None, None)
        n, k = lg[0].shape[0], lg[0].shape[2]
        with _C.on_device(dev):
            _C.check(_C.lib().d2amd_fcos_loss_backward(_ptrs(lg), _ptrs(dl), _ptrs(ct), _ptrs(anchors), *tg,
                                                       *[_C.ptr(u) for u in up], n, ctx.sizes, nl, k,
                                                       _C.dtype_code(lg[0]), cfg["norm"], cfg["alpha"], cfg["gamma"],
                                                       *[_ptrs(g) for g in grads], _C.stream()))
        return (None,) * (3 + nl) + tuple(grads[0]) + tuple(grads[1]) + tuple(grads[2])


def _loss_sums(op, anchors, pred_logits, pred_anchor_deltas, pred_centerness, targets, cfg):
    """Argument checks shared by the two forms; `targets(n, r, dev)` -> the tensors of `_FcosLoss`.
    -> (cls_sum, loc_sum, ctr_sum, stats)."""
    an = _anchors(anchors, op)
    nl = len(an)
    assert nl == len(pred_logits) == len(pred_anchor_deltas) == len(pred_centerness), \
        (nl, len(pred_logits), len(pred_anchor_deltas), len(pred_centerness))
    preds = (*pred_logits, *pred_anchor_deltas, *pred_centerness)
    if len({t.dtype for t in preds}) > 1:
        raise ValueError(f"{op}: logits, deltas and centerness of all levels must share one dtype")
    _C.require_gpu(*an, *preds, op=op)
    n = pred_logits[0].shape[0] if nl else 0
    r = sum(a.shape[0] for a in an)
    if n == 0 or r == 0:  # nothing to launch: zeros that still reach the inputs' graph
        dev = preds[0].device if preds else torch.device("cuda")
        zero = torch.zeros((), dtype=torch.float32, device=dev)
        for t in preds:
            zero = zero + t.sum().float() * 0
        return zero, zero.clone(), zero.clone(), torch.zeros(2, dtype=torch.int64, device=dev)
    k = pred_logits[0].shape[2]
    ct = [c.squeeze(-1) if c.dim() == 3 else c for c in pred_centerness]
    for a, x, d, c in zip(an, pred_logits, pred_anchor_deltas, ct):
        assert x.shape == (n, a.shape[0], k) and d.shape == (n, a.shape[0], 4) and c.shape == (n, a.shape[0]), \
            (a.shape, x.shape, d.shape, c.shape)
    dev = pred_logits[0].device
    an = [a.detach().to(dtype=torch.float32).contiguous() for a in an]
    return _FcosLoss.apply(cfg, targets(n, r, dev), nl, *an, *pred_logits, *pred_anchor_deltas, *ct)


def fcos_losses_from_gt(anchors: Sequence, pred_logits: List[torch.Tensor], pred_anchor_deltas: List[torch.Tensor],
                        pred_centerness: List[torch.Tensor], gt_boxes_list, gt_classes_list, *, num_classes: int,
                        center_sampling_radius: float = 1.5, normalize_by_size: bool = True, alpha: float,
                        gamma: float, gt_offsets=None):
    """The fused FCOS training losses, SUMMED (the caller normalises): matching, focal, GIoU and centerness in one launch.

    anchors[l] [A_l,4] (Tensor or Boxes); pred_logits[l] [N,A_l,K]; pred_anchor_deltas[l] [N,A_l,4]; pred_centerness[l]
    [N,A_l,1] or [N,A_l]; fp32, bf16 or fp16, one dtype for all predictions.  gt_boxes_list[i] [M_i,4] and
    gt_classes_list[i] [M_i] per image; or, with `gt_offsets` (int32 [N+1] on the device), the packed [G,4] boxes and [G]
    classes: then nothing is copied from the host and a captured graph replays with other offsets.
    alpha < 0: no alpha weighting.
    -> (loss_cls_sum, loss_loc_sum, loss_ctr_sum) fp32 scalars and stats int64[2] = (#positive points, N * R), on the
    device."""
    op = "fcos_losses_from_gt"
    if len(pred_logits):
        assert pred_logits[0].shape[-1] == num_classes, (pred_logits[0].shape, num_classes)
    cfg = dict(radius=float(center_sampling_radius), norm=int(bool(normalize_by_size)), alpha=float(alpha),
               gamma=float(gamma))

    def targets(n, r, dev):
        assert (len(gt_boxes_list) if gt_offsets is None else gt_offsets.numel() - 1) == n, "one ground truth per image"
        return _pack_gt(gt_boxes_list, gt_classes_list, gt_offsets, dev, op)

    return _loss_sums(op, anchors, pred_logits, pred_anchor_deltas, pred_centerness, targets, cfg)


def fcos_losses(anchors, pred_logits, gt_labels, pred_anchor_deltas, gt_boxes, pred_centerness, *, num_classes: int,
                normalizer: Union[float, torch.Tensor], focal_loss_alpha: float = 0.25, focal_loss_gamma: float = 2.0,
                normalize_by_size: bool = True):
    """`FCOS.losses` (fcos.py:193-238) -> {"loss_fcos_cls", "loss_fcos_loc", "loss_fcos_ctr"}, the reference's argument
    order.  gt_labels [N,R] and gt_boxes [N,R,4] (R = sum A_l), stacked or as the reference's lists of N tensors: a label
    in [0, num_classes) is positive, anything else background.  `normalizer`: a float or a 1-element device tensor, e.g.
    `ema_normalizer_(state, stats)` with `state` initialised to 300, FCOS' initial value (fcos.py:206; RetinaNet's is
    100); the division is a device op, nothing is read on the host."""
    op = "fcos_losses"
    if len(pred_logits):
        assert pred_logits[0].shape[-1] == num_classes, (pred_logits[0].shape, num_classes)
    cfg = dict(radius=0.0, norm=int(bool(normalize_by_size)), alpha=float(focal_loss_alpha),
               gamma=float(focal_loss_gamma))

    def targets(n, r, dev):
        given = [t for x in (gt_labels, gt_boxes) for t in ([x] if isinstance(x, torch.Tensor) else x)]
        _C.require_gpu(*[t for t in given if isinstance(t, torch.Tensor)], op=op)
        labels, boxes = _stacked(gt_labels, torch.int64, dev), _stacked(gt_boxes, torch.float32, dev)
        assert labels.shape == (n, r) and boxes.shape == (n, r, 4), (labels.shape, boxes.shape, n, r)
        return labels, boxes

    cls, loc, ctr, _ = _loss_sums(op, anchors, pred_logits, pred_anchor_deltas, pred_centerness, targets, cfg)
    if isinstance(normalizer, torch.Tensor):
        normalizer = normalizer.reshape(())
    return {"loss_fcos_cls": cls / normalizer, "loss_fcos_loc": loc / normalizer, "loss_fcos_ctr": ctr / normalizer}
