"""Keypoint-head glue of `detectron2.modeling.roi_heads.keypoint_head` on the hot path: `keypoint_rcnn_loss`
(keypoint_head.py:40-96) and `keypoint_rcnn_inference` (keypoint_head.py:99-132), same names, arguments and results,
backed by csrc/keypoint_head.hip:

* the loss computes the integer targets in the kernel, reads every valid row of logits once (no `nonzero`, no
  `pred[valid]` copy), counts the valid rows on the device and writes the whole gradient once in the backward;
* the inference decodes all ROIs in one launch (separable bicubic resize + argmax + score in LDS).

Neither reads anything on the host: both can be captured into a graph.
"""
import ctypes
from typing import List

import torch

from .. import _C
from ..structures.keypoints import heatmaps_to_keypoints

__all__ = ["keypoint_rcnn_loss", "keypoint_rcnn_inference", "keypoint_rcnn_loss_from_targets"]


class _KeypointLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, keypoints, rois, normalizer):
        n, k, s, _ = logits.shape
        x = logits.contiguous()
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        stats = torch.empty(1, dtype=torch.int64, device=x.device)
        L = _C.lib()
        ws_bytes = L.d2amd_keypoint_rcnn_loss_workspace_bytes(n * k)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
        with _C.on_device(x.device):
            _C.check(L.d2amd_keypoint_rcnn_loss_forward(_C.ptr(x), _C.ptr(keypoints), _C.ptr(rois), n, k, s,
                                                        _C.dtype_code(x), normalizer, _C.ptr(loss), _C.ptr(stats),
                                                        _C.ptr(ws), ctypes.c_size_t(ws_bytes), _C.stream()))
        # lse / target of every row and the valid count stay on the device, in `ws`
        ctx.save_for_backward(x, ws)
        ctx.normalizer = normalizer
        ctx.mark_non_differentiable(stats)
        ctx.set_materialize_grads(False)
        return loss, stats

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss, _grad_stats):
        if grad_loss is None:
            return None, None, None, None
        x, ws = ctx.saved_tensors
        n, k, s, _ = x.shape
        g = grad_loss.detach().to(dtype=torch.float32).contiguous()
        grad = torch.empty_like(x)
        with _C.on_device(x.device):
            _C.check(_C.lib().d2amd_keypoint_rcnn_loss_backward(_C.ptr(x), _C.ptr(ws), _C.ptr(g), n, k, s,
                                                                _C.dtype_code(x), ctx.normalizer, _C.ptr(grad),
                                                                _C.stream()))
        return grad, None, None, None


def keypoint_rcnn_loss_from_targets(pred_keypoint_logits: torch.Tensor, keypoints: torch.Tensor, boxes: torch.Tensor,
                                    normalizer=None):
    """Fused core of `keypoint_rcnn_loss`: (N, K, S, S) logits, (N, K, 3) keypoints (x, y, visibility), (N, 4) boxes ->
    (loss fp32 scalar, stats int64[1] on the device: the number of valid (n, k) rows).  normalizer None: the loss is
    divided by that number."""
    _C.require_gpu(pred_keypoint_logits, keypoints, boxes, op="keypoint_rcnn_loss")
    n, k = pred_keypoint_logits.shape[:2]
    assert pred_keypoint_logits.dim() == 4 and pred_keypoint_logits.size(2) == pred_keypoint_logits.size(3), \
        "Keypoint heatmaps must be square!"
    assert keypoints.shape == (n, k, 3) and boxes.shape == (n, 4), (keypoints.shape, boxes.shape, n, k)
    dev = pred_keypoint_logits.device
    kp = keypoints.detach().to(device=dev, dtype=torch.float32).contiguous()
    b = boxes.detach().to(device=dev, dtype=torch.float32).contiguous()
    return _KeypointLoss.apply(pred_keypoint_logits, kp, b, 0.0 if normalizer is None else float(normalizer))


def keypoint_rcnn_loss(pred_keypoint_logits: torch.Tensor, instances: List, normalizer):
    """Keypoint R-CNN loss: softmax cross-entropy over the S * S cells of every visible keypoint that lies in its
    proposal box, summed and divided by `normalizer` (None: the number of such keypoints).  `instances` are the
    reference's `Instances` (fields gt_keypoints with `.tensor`, proposal_boxes) or any objects with those attributes.
    No keypoint counts -> 0 (the reference also logs kpts_num_skipped_batches then, after a host sync)."""
    _C.require_gpu(pred_keypoint_logits, op="keypoint_rcnn_loss")
    kps, boxes = [], []
    for per_image in instances:
        if len(per_image) == 0:
            continue
        kps.append(per_image.gt_keypoints.tensor)
        boxes.append(per_image.proposal_boxes.tensor)
    if len(kps) == 0:
        return pred_keypoint_logits.sum() * 0
    loss, _ = keypoint_rcnn_loss_from_targets(pred_keypoint_logits, torch.cat(kps, dim=0), torch.cat(boxes, dim=0),
                                              normalizer)
    return loss


def keypoint_rcnn_inference(pred_keypoint_logits: torch.Tensor, pred_instances: List):
    """Attach `pred_keypoints` (n_i, K, 3) = (x, y, score) and `pred_keypoint_heatmaps` (n_i, K, S, S) to every element
    of `pred_instances` (objects with `pred_boxes.tensor` and `__len__`)."""
    _C.require_gpu(pred_keypoint_logits, op="keypoint_rcnn_inference")
    x = pred_keypoint_logits.detach()
    boxes = torch.cat([i.pred_boxes.tensor for i in pred_instances], dim=0).detach()
    res = heatmaps_to_keypoints(x, boxes)
    num = [len(i) for i in pred_instances]
    for kp, hm, inst in zip(res[:, :, [0, 1, 3]].split(num, dim=0), x.split(num, dim=0), pred_instances):
        inst.pred_keypoints = kp
        inst.pred_keypoint_heatmaps = hm
