"""Training losses of the dense-anchor detectors on the hot path: `RetinaNet.losses` (meta_arch/retinanet.py:160-210),
`RPN.losses` (proposal_generator/rpn.py:366-429) and the `_dense_box_regression_loss` both call
(box_regression.py:310-369), backed by csrc/dense_loss.hip:

* one forward and one backward launch for all images and levels: the per-level logits are never concatenated,
  mask-indexed or one-hot encoded; the targets come from the labels inside the kernel;
* the classification gradient is recomputed from the logits and every gradient element is written once;
* the foreground / valid counts stay on the device (`stats`): nothing here reads the host, so a training step that
  uses these losses can be captured into a graph.

`retinanet_label_anchors` and `ema_normalizer_` are the device forms of `RetinaNet.label_anchors`
(retinanet.py:212-255) and of `_ema_update("loss_normalizer", max(num_pos, 1), 100)` (retinanet.py:183,
dense_detector.py:160-181)."""
import ctypes
import math
from typing import List, Sequence, Union

import torch

from .. import _C

__all__ = ["dense_anchor_losses", "retinanet_losses", "rpn_losses", "retinanet_label_anchors", "ema_normalizer_",
           "DENSE_LOSS_TILE"]

DENSE_LOSS_TILE = 256  # anchors per workgroup (DL_TILE of csrc/dense_loss.hip)
_DEFAULT_SCALE_CLAMP = math.log(1000.0 / 16)
_LABEL_MODES = {"class": 0, "objectness": 1}
_BOX_LOSSES = {"smooth_l1": 0, "giou": 1}


def _ptrs(tensors):
    arr = (ctypes.c_void_p * max(len(tensors), 1))()
    for i, t in enumerate(tensors):
        arr[i] = t.data_ptr()
    return arr


class _DenseLoss(torch.autograd.Function):
    """(cfg, gt_labels [N,R], gt_boxes [N,R,4], L, *anchors, *logits, *deltas) -> (loss_cls_sum, loss_box_sum, stats)."""

    @staticmethod
    def forward(ctx, cfg, gt_labels, gt_boxes, nl, *levels):
        anchors, logits, deltas = levels[:nl], levels[nl:2 * nl], levels[2 * nl:]
        lg = [t.contiguous() for t in logits]
        dl = [t.contiguous() for t in deltas]
        dev = lg[0].device
        n, k = lg[0].shape[0], lg[0].shape[2]
        sizes = (ctypes.c_int * nl)(*[int(a.shape[0]) for a in anchors])
        wts = (ctypes.c_float * 4)(*cfg["weights"])
        scalars = (cfg["label_mode"], cfg["alpha"], cfg["gamma"], cfg["box_loss"], cfg["beta"], wts, cfg["scale_clamp"])
        loss_cls = torch.empty((), dtype=torch.float32, device=dev)
        loss_box = torch.empty((), dtype=torch.float32, device=dev)
        stats = torch.empty(2, dtype=torch.int64, device=dev)
        L = _C.lib()
        with _C.on_device(dev):
            ws_bytes = L.d2amd_dense_loss_workspace_bytes(n, sizes, nl)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            _C.check(L.d2amd_dense_loss_forward(_ptrs(lg), _ptrs(dl), _ptrs(anchors), _C.ptr(gt_labels), _C.ptr(gt_boxes),
                                                n, sizes, nl, k, _C.dtype_code(lg[0]), *scalars, _C.ptr(loss_cls),
                                                _C.ptr(loss_box), _C.ptr(stats), _C.ptr(ws), ctypes.c_size_t(ws_bytes),
                                                _C.stream()))
        # nothing per element is kept: the backward recomputes the gradient from the inputs
        ctx.save_for_backward(gt_labels, gt_boxes, *anchors, *lg, *dl)
        ctx.nl, ctx.sizes, ctx.scalars = nl, sizes, scalars
        ctx.mark_non_differentiable(stats)
        ctx.set_materialize_grads(False)
        return loss_cls, loss_box, stats

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_cls, grad_box, _grad_stats):
        nl = ctx.nl
        none = (None,) * (4 + 3 * nl)
        if grad_cls is None and grad_box is None:
            return none
        gt_labels, gt_boxes = ctx.saved_tensors[:2]
        lv = ctx.saved_tensors[2:]
        anchors, lg, dl = lv[:nl], lv[nl:2 * nl], lv[2 * nl:]
        dev = lg[0].device
        up = [torch.zeros((), dtype=torch.float32, device=dev) if g is None else
              g.detach().to(dtype=torch.float32).contiguous() for g in (grad_cls, grad_box)]
        g_lg = [torch.empty_like(t) for t in lg]
        g_dl = [torch.empty_like(t) for t in dl]
        n, k = lg[0].shape[0], lg[0].shape[2]
        with _C.on_device(dev):
            _C.check(_C.lib().d2amd_dense_loss_backward(_ptrs(lg), _ptrs(dl), _ptrs(anchors), _C.ptr(gt_labels),
                                                        _C.ptr(gt_boxes), _C.ptr(up[0]), _C.ptr(up[1]), n, ctx.sizes, nl,
                                                        k, _C.dtype_code(lg[0]), *ctx.scalars, _ptrs(g_lg), _ptrs(g_dl),
                                                        _C.stream()))
        return (None,) * (4 + nl) + tuple(g_lg) + tuple(g_dl)


def _tensor(x):
    return x if isinstance(x, torch.Tensor) else x.tensor


def _stacked(x, dtype, dev):
    if not isinstance(x, torch.Tensor):
        x = torch.stack([_tensor(t) for t in x])
    return x.detach().to(device=dev, dtype=dtype).contiguous()


def dense_anchor_losses(anchors: Sequence, pred_logits: List[torch.Tensor], pred_anchor_deltas: List[torch.Tensor],
                        gt_labels, gt_boxes, *, label_mode: str, alpha: float, gamma: float,
                        box_reg_loss_type: str = "smooth_l1", smooth_l1_beta: float = 0.0,
                        weights=(1.0, 1.0, 1.0, 1.0), scale_clamp: float = _DEFAULT_SCALE_CLAMP):
    """Fused classification + box-regression losses of a dense-anchor head, SUMMED (the caller normalises).

    anchors[l] [A_l,4] (Tensor or Boxes); pred_logits[l] [N,A_l,K] (or [N,A_l]: K = 1); pred_anchor_deltas[l] [N,A_l,4];
    gt_labels [N,R] and gt_boxes [N,R,4] (R = sum A_l), stacked or as the reference's lists of N tensors.
    label_mode "class": -1 ignore, K background, c < K foreground (RetinaNet); "objectness": -1 / 0 / 1 (RPN, K = 1).
    alpha < 0: no alpha weighting; gamma = 0: plain binary cross-entropy with logits.
    -> (loss_cls_sum, loss_box_sum) fp32 scalars and stats int64[2] = (#foreground rows, #valid rows), on the device."""
    if box_reg_loss_type not in _BOX_LOSSES:
        if box_reg_loss_type in ("diou", "ciou"):
            raise NotImplementedError(f"dense_anchor_losses: box_reg_loss_type '{box_reg_loss_type}' is not implemented "
                                      "(smooth_l1 and giou are)")
        raise ValueError(f"Invalid dense box regression loss type '{box_reg_loss_type}'")
    if label_mode not in _LABEL_MODES:
        raise ValueError(f"dense_anchor_losses: label_mode '{label_mode}' (class or objectness)")
    an = [_tensor(a) for a in anchors]
    if any(a.shape[-1] != 4 for a in an):
        raise NotImplementedError("dense_anchor_losses: 5-column (rotated) anchors are not implemented")
    nl = len(an)
    assert nl == len(pred_logits) == len(pred_anchor_deltas), (nl, len(pred_logits), len(pred_anchor_deltas))
    lg = [x.unsqueeze(-1) if x.dim() == 2 else x for x in pred_logits]
    given = [t for t in (*an, *lg, *pred_anchor_deltas, *([gt_labels] if isinstance(gt_labels, torch.Tensor) else gt_labels),
                         *([gt_boxes] if isinstance(gt_boxes, torch.Tensor) else gt_boxes)) if isinstance(t, torch.Tensor)]
    _C.require_gpu(*given, op="dense_anchor_losses")
    n = lg[0].shape[0] if nl else 0
    if n == 0 or sum(a.shape[0] for a in an) == 0:  # nothing to launch: zeros that still reach the inputs' graph
        dev = given[0].device if given else torch.device("cuda")
        zero = torch.zeros((), dtype=torch.float32, device=dev)
        for t in (*lg, *pred_anchor_deltas):
            zero = zero + t.sum().float() * 0
        return zero, zero.clone(), torch.zeros(2, dtype=torch.int64, device=dev)
    dev, k = lg[0].device, lg[0].shape[2]
    if len({t.dtype for t in (*lg, *pred_anchor_deltas)}) != 1:
        raise ValueError("dense_anchor_losses: logits and deltas of all levels must share one dtype")
    if label_mode == "objectness" and k != 1:
        raise ValueError(f"dense_anchor_losses: objectness labels need K = 1, got {k}")
    r = sum(a.shape[0] for a in an)
    for a, x, d in zip(an, lg, pred_anchor_deltas):
        assert x.shape == (n, a.shape[0], k) and d.shape == (n, a.shape[0], 4), (a.shape, x.shape, d.shape)
    labels = _stacked(gt_labels, torch.int64, dev)
    boxes = _stacked(gt_boxes, torch.float32, dev)
    assert labels.shape == (n, r) and boxes.shape == (n, r, 4), (labels.shape, boxes.shape, n, r)
    cfg = dict(label_mode=_LABEL_MODES[label_mode], alpha=float(alpha), gamma=float(gamma),
               box_loss=_BOX_LOSSES[box_reg_loss_type], beta=float(smooth_l1_beta),
               weights=[float(w) for w in weights], scale_clamp=float(scale_clamp))
    an = [a.detach().to(dtype=torch.float32).contiguous() for a in an]
    return _DenseLoss.apply(cfg, labels, boxes, nl, *an, *lg, *pred_anchor_deltas)


def retinanet_losses(anchors, pred_logits, gt_labels, pred_anchor_deltas, gt_boxes, *, num_classes: int,
                     normalizer: Union[float, torch.Tensor], focal_loss_alpha: float = 0.25,
                     focal_loss_gamma: float = 2.0, box_reg_loss_type: str = "smooth_l1", smooth_l1_beta: float = 0.0,
                     box2box_weights=(1.0, 1.0, 1.0, 1.0), scale_clamp: float = _DEFAULT_SCALE_CLAMP):
    """`RetinaNet.losses` (retinanet.py:160-210) -> {"loss_cls", "loss_box_reg"}.  `normalizer`: a float or a 1-element
    device tensor (e.g. `ema_normalizer_`'s result); the division is a device op, nothing is read on the host."""
    if len(pred_logits):
        assert pred_logits[0].shape[-1] == num_classes, (pred_logits[0].shape, num_classes)
    cls, box, _ = dense_anchor_losses(anchors, pred_logits, pred_anchor_deltas, gt_labels, gt_boxes, label_mode="class",
                                      alpha=focal_loss_alpha, gamma=focal_loss_gamma,
                                      box_reg_loss_type=box_reg_loss_type, smooth_l1_beta=smooth_l1_beta,
                                      weights=box2box_weights, scale_clamp=scale_clamp)
    if isinstance(normalizer, torch.Tensor):
        normalizer = normalizer.reshape(())
    return {"loss_cls": cls / normalizer, "loss_box_reg": box / normalizer}


def rpn_losses(anchors, pred_objectness_logits, gt_labels, pred_anchor_deltas, gt_boxes, *, batch_size_per_image: int,
               box_reg_loss_type: str = "smooth_l1", smooth_l1_beta: float = 0.0, box2box_weights=(1.0, 1.0, 1.0, 1.0),
               loss_weight=1.0, scale_clamp: float = _DEFAULT_SCALE_CLAMP):
    """`RPN.losses` (rpn.py:366-429) -> {"loss_rpn_cls", "loss_rpn_loc"}: BCE with logits over the rows labelled 0 / 1,
    the box term over the rows labelled 1, both divided by batch_size_per_image * N and weighted by `loss_weight` (a
    float for both, or the reference's dict by loss name)."""
    cls, box, _ = dense_anchor_losses(anchors, pred_objectness_logits, pred_anchor_deltas, gt_labels, gt_boxes,
                                      label_mode="objectness", alpha=-1.0, gamma=0.0,
                                      box_reg_loss_type=box_reg_loss_type, smooth_l1_beta=smooth_l1_beta,
                                      weights=box2box_weights, scale_clamp=scale_clamp)
    num_images = len(gt_labels)
    normalizer = float(batch_size_per_image * max(num_images, 1))
    losses = {"loss_rpn_cls": cls / normalizer, "loss_rpn_loc": box / normalizer}
    if not isinstance(loss_weight, dict):
        loss_weight = {"loss_rpn_cls": float(loss_weight), "loss_rpn_loc": float(loss_weight)}
    return {name: v * loss_weight.get(name, 1.0) for name, v in losses.items()}


@torch.no_grad()
def retinanet_label_anchors(anchors, gt_boxes_list, gt_classes_list, matcher, num_classes: int):
    """`RetinaNet.label_anchors` (retinanet.py:212-255) for the batch: the images' ground truth is matched against the
    concatenated anchors in one `Matcher.match_boxes_batch`, the rest are device-side index ops.
    -> (gt_labels [N,R] int64: -1 ignore, num_classes background, else the matched class; gt_boxes [N,R,4] fp32).
    An image without ground truth: all background, zero boxes."""
    an = torch.cat([_tensor(a) for a in anchors], dim=0)
    gts = [_tensor(g).reshape(-1, 4) for g in gt_boxes_list]
    _C.require_gpu(an, *gts, *gt_classes_list, op="retinanet_label_anchors")
    n, r = len(gts), an.shape[0]
    labels = torch.full((n, r), num_classes, dtype=torch.int64, device=an.device)
    boxes = torch.zeros((n, r, 4), dtype=torch.float32, device=an.device)
    some = [i for i in range(n) if gts[i].shape[0] > 0]  # (shapes: host knowledge, no device read)
    if some and r > 0:
        matched, quality = matcher.match_boxes_batch([gts[i] for i in some], an)
        for row, i in enumerate(some):
            boxes[i] = gts[i].float().index_select(0, matched[row])
            cls = gt_classes_list[i].to(torch.int64).index_select(0, matched[row])
            cls = torch.where(quality[row] == 0, num_classes, cls)
            labels[i] = torch.where(quality[row] == -1, -1, cls)
    return labels, boxes


@torch.no_grad()
def ema_normalizer_(state: torch.Tensor, stats: torch.Tensor, momentum: float = 0.9):
    """state <- state * momentum + max(stats[0], 1) * (1 - momentum), in place on the 1-element device tensor `state`
    (initialise it to 100, the reference's initial value).  -> a copy of the new value: what this iteration's losses
    are divided by (the copy keeps autograd's saved divisor apart from the next in-place update)."""
    _C.require_gpu(state, stats, op="ema_normalizer_")
    num_pos = stats[0].clamp(min=1).to(state.dtype)
    state.mul_(momentum).add_(num_pos * (1.0 - momentum))
    return state.clone()
