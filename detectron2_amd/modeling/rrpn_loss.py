"""Training half of the rotated proposal generator (proposal_generator/rrpn.py) on the hot path:

* `rrpn_label_anchors`: `RRPN.label_and_sample_anchors` (rrpn.py:151-200) without its subsampling -- the batch's
  ground truth against the concatenated rotated anchors in one `Matcher.match_boxes_rotated_batch`
  (csrc/matcher_rot.hip), no M x N matrix;
* `rrpn_losses`: `RPN.losses` (rpn.py:366-429) as RRPN inherits it with `Box2BoxTransformRotated.get_deltas`
  (box_regression.py:145-181), backed by csrc/rrpn_loss.hip: one forward and one backward launch for all images and
  levels, targets computed in the kernel, every gradient element written once, sums reduced in a fixed order, nothing
  read on the host."""
import ctypes

import torch

from .. import _C
from .dense_loss import _ptrs, _stacked, _tensor

__all__ = ["rrpn_losses", "rrpn_label_anchors", "MATCH_ROTATED_STRIP", "MATCH_ROTATED_GT_CHUNK"]

MATCH_ROTATED_STRIP = 128     # boxes per workgroup (MR_STRIP of csrc/matcher_rot.hip)
MATCH_ROTATED_GT_CHUNK = 64   # ground-truth boxes staged per LDS pass (MR_CHUNK)


class _RrpnLoss(torch.autograd.Function):
    """(beta, weights, gt_labels int8 [N,R], gt_boxes [N,R,5], L, *anchors, *logits, *deltas) -> (cls_sum, box_sum)."""

    @staticmethod
    def forward(ctx, beta, weights, gt_labels, gt_boxes, nl, *levels):
        anchors, logits, deltas = levels[:nl], levels[nl:2 * nl], levels[2 * nl:]
        lg = [t.contiguous() for t in logits]
        dl = [t.contiguous() for t in deltas]
        dev = lg[0].device
        n = lg[0].shape[0]
        sizes = (ctypes.c_int * nl)(*[int(a.shape[0]) for a in anchors])
        scalars = (_C.dtype_code(lg[0]), beta, (ctypes.c_float * 5)(*weights))
        loss_cls = torch.empty((), dtype=torch.float32, device=dev)
        loss_box = torch.empty((), dtype=torch.float32, device=dev)
        stats = torch.empty(2, dtype=torch.int64, device=dev)
        L = _C.lib()
        with _C.on_device(dev):
            ws_bytes = L.d2amd_rrpn_loss_workspace_bytes(n, sizes, nl)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            _C.check(L.d2amd_rrpn_loss_forward(_ptrs(lg), _ptrs(dl), _ptrs(anchors), _C.ptr(gt_labels), _C.ptr(gt_boxes),
                                               n, sizes, nl, *scalars, _C.ptr(loss_cls), _C.ptr(loss_box), _C.ptr(stats),
                                               _C.ptr(ws), ctypes.c_size_t(ws_bytes), _C.stream()))
        # nothing per element is kept: the backward recomputes the gradient from the inputs
        ctx.save_for_backward(gt_labels, gt_boxes, *anchors, *lg, *dl)
        ctx.nl, ctx.sizes, ctx.scalars = nl, sizes, scalars
        ctx.set_materialize_grads(False)
        return loss_cls, loss_box

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_cls, grad_box):
        nl = ctx.nl
        if grad_cls is None and grad_box is None:
            return (None,) * (5 + 3 * nl)
        gt_labels, gt_boxes = ctx.saved_tensors[:2]
        lv = ctx.saved_tensors[2:]
        anchors, lg, dl = lv[:nl], lv[nl:2 * nl], lv[2 * nl:]
        dev = lg[0].device
        up = [torch.zeros((), dtype=torch.float32, device=dev) if g is None else
              g.detach().to(dtype=torch.float32).contiguous() for g in (grad_cls, grad_box)]
        g_lg = [torch.empty_like(t) for t in lg]
        g_dl = [torch.empty_like(t) for t in dl]
        with _C.on_device(dev):
            _C.check(_C.lib().d2amd_rrpn_loss_backward(_ptrs(lg), _ptrs(dl), _ptrs(anchors), _C.ptr(gt_labels),
                                                       _C.ptr(gt_boxes), _C.ptr(up[0]), _C.ptr(up[1]), lg[0].shape[0],
                                                       ctx.sizes, nl, *ctx.scalars, _ptrs(g_lg), _ptrs(g_dl), _C.stream()))
        return (None,) * (5 + nl) + tuple(g_lg) + tuple(g_dl)


def rrpn_losses(anchors, pred_objectness_logits, gt_labels, pred_anchor_deltas, gt_boxes, *, batch_size_per_image: int,
                smooth_l1_beta: float = 0.0, box2box_weights=(1.0, 1.0, 1.0, 1.0, 1.0), loss_weight=1.0):
    """`RPN.losses` (rpn.py:366-429) for rotated anchors -> {"loss_rpn_cls", "loss_rpn_loc"}.

    anchors[l] [A_l,5] (Tensor or RotatedBoxes) rows (cx, cy, w, h, angle in degrees); pred_objectness_logits[l] [N,A_l]
    (or [N,A_l,1]) and pred_anchor_deltas[l] [N,A_l,5] in fp32 / fp16 / bf16; gt_labels [N,R] with -1 ignore /
    0 background / 1 foreground and gt_boxes [N,R,5] (R = sum A_l), stacked or as the reference's lists of N tensors.
    BCE with logits over the rows labelled 0 / 1, smooth-L1 (the only rotated box loss of the reference) of the deltas
    against `Box2BoxTransformRotated.get_deltas` over the rows labelled 1; both divided by batch_size_per_image * N and
    weighted by `loss_weight` (a float for both, or the reference's dict by loss name), exactly as `rpn_losses`."""
    an = [_tensor(a) for a in anchors]
    nl = len(an)
    assert nl == len(pred_objectness_logits) == len(pred_anchor_deltas), (nl, len(pred_objectness_logits), len(pred_anchor_deltas))
    lg = [x.squeeze(-1) if x.dim() == 3 else x for x in pred_objectness_logits]
    dl = list(pred_anchor_deltas)
    given = [t for t in (*an, *lg, *dl, *([gt_labels] if isinstance(gt_labels, torch.Tensor) else gt_labels),
                         *([gt_boxes] if isinstance(gt_boxes, torch.Tensor) else gt_boxes)) if isinstance(t, torch.Tensor)]
    _C.require_gpu(*given, op="rrpn_losses")
    if any(a.dim() != 2 or a.shape[1] != 5 for a in an):
        raise ValueError("rrpn_losses: anchors must be [A_l, 5] rotated boxes (rpn_losses takes 4-column boxes)")
    if len(box2box_weights) != 5:
        raise ValueError("rrpn_losses: box2box_weights must be (wx, wy, ww, wh, wa)")
    num_images = len(gt_labels)
    normalizer = float(batch_size_per_image * max(num_images, 1))
    n = lg[0].shape[0] if nl else 0
    r = sum(a.shape[0] for a in an)
    if n == 0 or r == 0:  # nothing to launch: zeros that still reach the inputs' graph
        dev = given[0].device if given else torch.device("cuda")
        cls = torch.zeros((), dtype=torch.float32, device=dev)
        for t in (*lg, *dl):
            cls = cls + t.sum().float() * 0
        box = cls.clone()
    else:
        dev = lg[0].device
        if len({t.dtype for t in (*lg, *dl)}) != 1:
            raise ValueError("rrpn_losses: logits and deltas of all levels must share one dtype")
        for a, x, d in zip(an, lg, dl):
            assert x.shape == (n, a.shape[0]) and d.shape == (n, a.shape[0], 5), (a.shape, x.shape, d.shape)
        labels = _stacked(gt_labels, torch.int8, dev)
        boxes = _stacked(gt_boxes, torch.float32, dev)
        assert labels.shape == (n, r) and boxes.shape == (n, r, 5), (labels.shape, boxes.shape, n, r)
        an = [a.detach().to(dtype=torch.float32).contiguous() for a in an]
        cls, box = _RrpnLoss.apply(float(smooth_l1_beta), [float(w) for w in box2box_weights], labels, boxes, nl,
                                   *an, *lg, *dl)
    losses = {"loss_rpn_cls": cls / normalizer, "loss_rpn_loc": box / normalizer}
    if not isinstance(loss_weight, dict):
        loss_weight = {"loss_rpn_cls": float(loss_weight), "loss_rpn_loc": float(loss_weight)}
    return {name: v * loss_weight.get(name, 1.0) for name, v in losses.items()}


@torch.no_grad()
def rrpn_label_anchors(anchors, gt_boxes_list, matcher):
    """`RRPN.label_and_sample_anchors` (rrpn.py:151-200) for the batch, WITHOUT the subsampling: the images' ground truth
    is matched against the concatenated rotated anchors in one `Matcher.match_boxes_rotated_batch`.
    -> (gt_labels [N,R] int8: the matcher's labels; matched_gt_boxes [N,R,5] fp32).  An image without ground truth gets
    all-zero boxes and the matcher's labels for no ground truth (rrpn.py:178-197).
    Subsampling stays with `subsample_anchor_labels_(gt_labels, batch_size_per_image, positive_fraction)`, which rewrites
    these labels in place."""
    an = torch.cat([_tensor(a) for a in anchors], dim=0)
    gts = [_tensor(g).reshape(-1, 5) for g in gt_boxes_list]
    _C.require_gpu(an, *gts, op="rrpn_label_anchors")
    n, r = len(gts), an.shape[0]
    matched, labels = matcher.match_boxes_rotated_batch(gts, an)
    boxes = torch.zeros((n, r, 5), dtype=torch.float32, device=an.device)
    for i in range(n):
        if gts[i].shape[0] > 0 and r > 0:  # (shapes: host knowledge, no device read)
            boxes[i] = gts[i].float().index_select(0, matched[i])
    return labels, boxes
