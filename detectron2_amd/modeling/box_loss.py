"""Training loss of the box head on the hot path: `FastRCNNOutputLayers.losses` (roi_heads/fast_rcnn.py:307-352) with its
`_log_classification_stats` (:88-115), `sigmoid_cross_entropy_loss` (:386-422) and `box_reg_loss` (:424-463), backed by
csrc/box_loss.hip:

* one forward launch set (loss kernel + a one-workgroup reduction) and one backward launch; no argmax / nonzero / gather
  / one-hot, nothing per element saved for the backward;
* rows whose class is outside [0, K] -- the `-1` padding of `label_and_sample_proposals_fixed` -- count for nothing: the
  normaliser is the number of the other rows, counted on the device, so the sampler's fixed-shape result is consumed as
  it is (`gt_index` / `gt_offsets` / `rows_per_image`: the matched boxes are read from the stacked ground truth inside
  the kernel);
* the five classification statistics stay on the device: nothing here reads the host, so the connected training step
  can be captured into a graph."""
import ctypes
import math

import torch

from .. import _C

__all__ = ["fast_rcnn_losses", "fast_rcnn_losses_with_stats"]

_DEFAULT_SCALE_CLAMP = math.log(1000.0 / 16)
_BOX_LOSSES = {"smooth_l1": 0, "giou": 1}


class _BoxLoss(torch.autograd.Function):
    """(cfg, scores [R,K+1], deltas [R,4 | 4K], gt_classes [R], proposal_boxes [R,4], gt_boxes, gt_index, gt_offsets,
    class_weight) -> (loss_cls, loss_box_reg, stats[5])."""

    @staticmethod
    def forward(ctx, cfg, scores, deltas, gt_classes, proposal_boxes, gt_boxes, gt_index, gt_offsets, class_weight):
        sc, dl = scores.contiguous(), deltas.contiguous()
        dev, r, k = sc.device, sc.shape[0], sc.shape[1] - 1
        wts = (ctypes.c_float * 4)(*cfg["weights"])
        shape = (r, k, dl.shape[1], cfg["rows_per_image"], 0 if gt_offsets is None else gt_offsets.shape[0],
                 gt_boxes.shape[0], _C.dtype_code(sc), cfg["cls_loss"])
        tail = (_C.ptr(class_weight), cfg["box_loss"], cfg["beta"], wts, cfg["scale_clamp"])
        inputs = (_C.ptr(sc), _C.ptr(dl), _C.ptr(gt_classes), _C.ptr(proposal_boxes), _C.ptr(gt_boxes), _C.ptr(gt_index),
                  _C.ptr(gt_offsets))
        losses = torch.empty(2, dtype=torch.float32, device=dev)
        stats = torch.empty(5, dtype=torch.int64, device=dev)
        L = _C.lib()
        with _C.on_device(dev):
            ws_bytes = L.d2amd_fast_rcnn_loss_workspace_bytes(r)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            _C.check(L.d2amd_fast_rcnn_loss_forward(*inputs, *shape, *tail, _C.ptr(losses), _C.ptr(stats), _C.ptr(ws),
                                                    ctypes.c_size_t(ws_bytes), _C.stream()))
        # the backward recomputes the gradient from the inputs and the workspace's row count and per-row (max, sum)
        ctx.save_for_backward(sc, dl, gt_classes, proposal_boxes, gt_boxes, gt_index, gt_offsets, class_weight, ws)
        ctx.shape, ctx.tail = shape, tail[1:]
        ctx.mark_non_differentiable(stats)
        ctx.set_materialize_grads(False)
        return losses[0], losses[1], stats

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_cls, grad_box, _grad_stats):
        if grad_cls is None and grad_box is None:
            return (None,) * 9
        sc, dl, gt_classes, proposal_boxes, gt_boxes, gt_index, gt_offsets, class_weight, ws = ctx.saved_tensors
        dev = sc.device
        up = [torch.zeros((), dtype=torch.float32, device=dev) if g is None else
              g.detach().to(dtype=torch.float32).contiguous() for g in (grad_cls, grad_box)]
        g_sc, g_dl = torch.empty_like(sc), torch.empty_like(dl)
        with _C.on_device(dev):
            _C.check(_C.lib().d2amd_fast_rcnn_loss_backward(
                _C.ptr(sc), _C.ptr(dl), _C.ptr(gt_classes), _C.ptr(proposal_boxes), _C.ptr(gt_boxes), _C.ptr(gt_index),
                _C.ptr(gt_offsets), _C.ptr(up[0]), _C.ptr(up[1]), *ctx.shape, _C.ptr(class_weight), *ctx.tail, _C.ptr(ws),
                ctypes.c_size_t(ws.numel()), _C.ptr(g_sc), _C.ptr(g_dl), _C.stream()))
        return (None, g_sc, g_dl) + (None,) * 6


def _tensor(x):
    return x if isinstance(x, torch.Tensor) else x.tensor


def fast_rcnn_losses_with_stats(scores, proposal_deltas, gt_classes, proposal_boxes, gt_boxes, *, gt_index=None,
                                gt_offsets=None, rows_per_image=None, box_reg_loss_type: str = "smooth_l1",
                                smooth_l1_beta: float = 0.0, box2box_weights=(10.0, 10.0, 5.0, 5.0),
                                scale_clamp: float = _DEFAULT_SCALE_CLAMP, loss_weight=1.0, use_sigmoid_ce: bool = False,
                                class_weight=None):
    """`FastRCNNOutputLayers.losses` fused.  scores [R, K+1] (last column: background) and proposal_deltas [R, 4] or
    [R, 4K], one floating dtype; gt_classes [R] (any leading shape, e.g. the sampler's [N, S]): [0, K) foreground, K
    background, anything else (-1) PADDING -- no loss, no statistic, zero gradient, left out of the normaliser, which is
    the number of the other rows (the reference's `gt_classes.numel()` when nothing is padded); proposal_boxes [R, 4]
    (or [N, S, 4], or Boxes).  The matched ground truth, either
      gt_boxes [R, 4]: one box per row, the reference's form, or
      the sampler's form: gt_boxes the stacked [G, 4] table (or the list of the images' [G_i, 4] tensors / Boxes, which
      is concatenated here), gt_index [R] the row's match inside its image, rows_per_image = S (image n owns rows n S ...
      n S + S - 1) and gt_offsets int64 [N], image n's first row of the table (default: from the list's lengths).  With
      `out = label_and_sample_proposals_fixed(...)`: gt_classes=out["classes"], proposal_boxes=out["boxes"],
      gt_index=out["gt_index"], rows_per_image=S, gt_boxes=<the list given to the sampler>.
    box_reg_loss_type smooth_l1 (beta = 0: L1) or giou (diou / ciou and 5-column boxes raise NotImplementedError);
    use_sigmoid_ce: BCE over the first K columns, times class_weight fp32 [K] when given (the federated-loss class mask;
    which classes it holds is the caller's business).  loss_weight: a float for both losses or the reference's dict.
    -> ({"loss_cls", "loss_box_reg"}, stats int64 [5] on the device = rows that count, foreground rows, argmax == class,
    foreground with argmax == class, foreground predicted as background; argmax ties go to the lowest index)."""
    if box_reg_loss_type not in _BOX_LOSSES:
        if box_reg_loss_type in ("diou", "ciou"):
            raise NotImplementedError(f"fast_rcnn_losses: box_reg_loss_type '{box_reg_loss_type}' is not implemented "
                                      "(smooth_l1 and giou are)")
        raise ValueError(f"Invalid bbox reg loss type '{box_reg_loss_type}'")
    boxes = _tensor(proposal_boxes)
    if boxes.shape[-1] != 4:
        raise NotImplementedError("fast_rcnn_losses: 5-column (rotated) boxes are not implemented")
    table = gt_boxes
    if isinstance(gt_boxes, (list, tuple)):
        parts = [_tensor(g).reshape(-1, 4) for g in gt_boxes]
        table = torch.cat(parts) if parts else boxes.new_zeros((0, 4))
        if gt_index is not None and gt_offsets is None:  # (shapes: host knowledge; made once per call, not a device read)
            sizes = [0] + [int(g.shape[0]) for g in parts[:-1]]
            gt_offsets = torch.tensor(sizes, dtype=torch.int64).cumsum(0).to(table.device, non_blocking=True)
    table = _tensor(table)
    _C.require_gpu(scores, proposal_deltas, gt_classes, boxes, table, gt_index, gt_offsets, class_weight,
                   op="fast_rcnn_losses")
    assert scores.dim() == 2 and proposal_deltas.dim() == 2 and scores.shape[1] >= 2, (scores.shape, proposal_deltas.shape)
    if scores.dtype != proposal_deltas.dtype:
        raise ValueError("fast_rcnn_losses: scores and proposal_deltas must share one dtype")
    r, k, dev = scores.shape[0], scores.shape[1] - 1, scores.device
    if proposal_deltas.shape[1] not in (4, 4 * k) or proposal_deltas.shape[0] != r:
        raise ValueError(f"fast_rcnn_losses: proposal_deltas {tuple(proposal_deltas.shape)} for scores {tuple(scores.shape)}")
    if not isinstance(loss_weight, dict):
        loss_weight = {"loss_cls": float(loss_weight), "loss_box_reg": float(loss_weight)}
    scale = lambda name, v: v if loss_weight.get(name, 1.0) == 1.0 else v * loss_weight.get(name, 1.0)
    if r == 0:  # nothing to launch: zeros that still reach the inputs' graph (the reference's `input.sum() * 0`)
        zero = scores.sum().float() * 0 + proposal_deltas.sum().float() * 0
        return ({"loss_cls": scale("loss_cls", zero), "loss_box_reg": scale("loss_box_reg", zero.clone())},
                torch.zeros(5, dtype=torch.int64, device=dev))
    classes = gt_classes.detach().to(torch.int64).reshape(-1).contiguous()
    boxes = boxes.detach().to(torch.float32).reshape(-1, 4).contiguous()
    table = table.detach().to(torch.float32).reshape(-1, 4).contiguous()
    assert classes.shape[0] == r and boxes.shape[0] == r, (classes.shape, boxes.shape, r)
    if gt_index is None:
        assert table.shape[0] == r, (table.shape, r)
        rows_per_image = 0
    else:
        assert gt_offsets is not None and rows_per_image, "the gt_index form needs gt_offsets and rows_per_image"
        gt_index = gt_index.detach().to(torch.int64).reshape(-1).contiguous()
        gt_offsets = gt_offsets.detach().to(torch.int64).reshape(-1).contiguous()
        assert gt_index.shape[0] == r and gt_offsets.shape[0] * int(rows_per_image) >= r, (gt_index.shape, gt_offsets.shape)
        if table.shape[0] == 0:  # (no ground truth anywhere: no row is foreground; one row for the kernel's clamp)
            table = table.new_zeros((1, 4))
    if class_weight is not None:
        if not use_sigmoid_ce:
            raise ValueError("fast_rcnn_losses: class_weight belongs to use_sigmoid_ce")
        class_weight = class_weight.detach().to(torch.float32).reshape(-1).contiguous()
        assert class_weight.shape[0] == k, (class_weight.shape, k)
    cfg = dict(cls_loss=int(bool(use_sigmoid_ce)), box_loss=_BOX_LOSSES[box_reg_loss_type], beta=float(smooth_l1_beta),
               weights=[float(w) for w in box2box_weights], scale_clamp=float(scale_clamp),
               rows_per_image=int(rows_per_image or 0))
    cls, box, stats = _BoxLoss.apply(cfg, scores, proposal_deltas, classes, boxes, table, gt_index, gt_offsets, class_weight)
    return {"loss_cls": scale("loss_cls", cls), "loss_box_reg": scale("loss_box_reg", box)}, stats


def fast_rcnn_losses(scores, proposal_deltas, gt_classes, proposal_boxes, gt_boxes, **kwargs):
    """`fast_rcnn_losses_with_stats` without the statistics: -> {"loss_cls", "loss_box_reg"}."""
    return fast_rcnn_losses_with_stats(scores, proposal_deltas, gt_classes, proposal_boxes, gt_boxes, **kwargs)[0]
