"""The Panoptic FPN merge of `detectron2.modeling.meta_arch.panoptic_fpn` on the hot path, backed by csrc/panoptic.hip:

* `combine_semantic_and_instance_outputs`: the reference's function (panoptic_fpn.py:184-269) under its own name,
  arguments and return value.  The reference loops over the detections on the host (three `.item()` reads and about six
  full-image launches each, then `torch.unique(...).cpu()` and a read per stuff class); here the image is merged by four
  launches and ONE host transfer, of the small segment table the dicts are built from.
* `panoptic_combine_device`: the same merge with every result left on the device at fixed shapes, no host read.  It also
  takes the mask head's soft masks and the boxes in place of pasted masks: the paste sample is evaluated inside the
  kernel, and no (R, H, W) mask is ever allocated.
"""
import ctypes
from typing import Dict, List, Optional, Tuple

import torch

from .. import _C

__all__ = ["combine_semantic_and_instance_outputs", "panoptic_combine_device"]

MAX_DETECTIONS = 128
MAX_CLASSES = 256


def _combine(scores, pred_classes, semantic_results, overlap_threshold, stuff_area_thresh, instances_score_thresh,
             pred_masks, mask_probs, boxes, mask_threshold, num_classes):
    """-> (panoptic_seg, ONE int64 tensor holding the segment rows, the count and the stats, the number of rows)"""
    if (pred_masks is None) == (mask_probs is None):
        raise ValueError("panoptic_combine_device: pass exactly one of pred_masks and mask_probs")
    if mask_probs is not None and boxes is None:
        raise ValueError("panoptic_combine_device: mask_probs need boxes")
    boxes = getattr(boxes, "tensor", boxes) if mask_probs is not None else None
    _C.require_gpu(scores, pred_classes, semantic_results, pred_masks, mask_probs, boxes, op="panoptic_combine")
    assert semantic_results.dim() == 2, f"panoptic_combine: semantic_results must be (H, W), got {tuple(semantic_results.shape)}"
    h, w = semantic_results.shape
    r = scores.shape[0]
    assert pred_classes.shape[0] == r, (tuple(pred_classes.shape), r)
    dev = semantic_results.device
    sem = semantic_results.detach()
    sem = (sem if sem.dtype == torch.int64 else sem.long()).contiguous()
    sc = scores.detach().float().contiguous()
    cls = pred_classes.detach().long().contiguous()
    masks = probs = bx = None
    m, dtype = 1, _C.F32
    if pred_masks is not None:
        assert tuple(pred_masks.shape) == (r, h, w), (tuple(pred_masks.shape), (r, h, w))
        if pred_masks.dtype not in (torch.bool, torch.uint8):
            raise NotImplementedError(f"panoptic_combine: pred_masks of {pred_masks.dtype} (bool and uint8 are implemented)")
        masks = pred_masks.detach().contiguous()
        masks = masks.view(torch.uint8) if masks.dtype == torch.bool else masks
    else:
        probs = mask_probs.detach()
        probs = probs[:, 0] if probs.dim() == 4 else probs
        assert probs.dim() == 3 and probs.shape[0] == r and probs.shape[1] == probs.shape[2], tuple(mask_probs.shape)
        if probs.dtype not in _C._DTYPES:
            raise NotImplementedError(f"panoptic_combine: mask_probs of {probs.dtype} (fp32, f16 and bf16 are implemented)")
        if not mask_threshold >= 0:
            raise ValueError("panoptic_combine: mask_threshold must be >= 0")
        probs = probs.contiguous()
        m, dtype = probs.shape[1], _C.dtype_code(probs)
        bx = boxes.detach().float().contiguous()
        assert tuple(bx.shape) == (r, 4), tuple(bx.shape)
    L = _C.lib()
    n_rows = r + max(int(num_classes), 0)
    seg = torch.empty((h, w), dtype=torch.int32, device=dev)
    out = torch.empty(n_rows * 5 + 2, dtype=torch.int64, device=dev)  # segments, count, stats: one allocation
    ws_bytes = L.d2amd_panoptic_workspace_bytes(h, w, r)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    with _C.on_device(dev):
        rc = L.d2amd_panoptic_combine(
            _C.ptr(sc), _C.ptr(cls), _C.ptr(sem), _C.ptr(masks), _C.ptr(probs), _C.ptr(bx), r, h, w, m, dtype,
            float(mask_threshold), float(overlap_threshold), float(stuff_area_thresh), float(instances_score_thresh),
            int(num_classes), _C.ptr(seg), _C.ptr(out), ctypes.c_void_p(out.data_ptr() + n_rows * 40),
            ctypes.c_void_p(out.data_ptr() + n_rows * 40 + 8), _C.ptr(ws), ctypes.c_size_t(ws_bytes), _C.stream())
    if rc == _C.EUNSUPPORTED:  # made before any launch
        raise NotImplementedError(L.d2amd_last_error().decode())
    _C.check(rc)
    return seg, out, n_rows


def panoptic_combine_device(scores: torch.Tensor, pred_classes: torch.Tensor, semantic_results: torch.Tensor,
                            overlap_threshold: float, stuff_area_thresh: float, instances_score_thresh: float, *,
                            pred_masks: Optional[torch.Tensor] = None, mask_probs: Optional[torch.Tensor] = None,
                            boxes: Optional[torch.Tensor] = None, mask_threshold: float = 0.5,
                            num_classes: int = MAX_CLASSES) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """-> (panoptic_seg int32 (H, W), segments int64 (R + num_classes, 5), count int64 (1,), stats int64 (1,)), all on
    the device.  `segments` rows are (id, isthing, category_id, instance index or -1, area) in id order -- a thing's area
    is what it keeps after truncation -- zeros behind the first `count`.  `stats`: pixels whose label is outside
    [0, num_classes): they get no stuff segment (`sem_seg_loss_with_stats`' convention).

    Exactly one mask source: `pred_masks` (R, H, W) bool / uint8 as `detector_postprocess` yields them, or `mask_probs`
    (R, M, M) / (R, 1, M, M) fp32 / f16 / bf16 with `boxes` (R, 4) in output-image coordinates -- a pixel is then covered
    exactly where `paste_masks_in_image(mask_probs, boxes, (H, W), mask_threshold)` is True.  More than 128 detections,
    more than 256 classes or a mask above 90 x 90 raise NotImplementedError."""
    seg, out, n = _combine(scores, pred_classes, semantic_results, overlap_threshold, stuff_area_thresh,
                           instances_score_thresh, pred_masks, mask_probs, boxes, mask_threshold, num_classes)
    return seg, out[:n * 5].view(n, 5), out[n * 5:n * 5 + 1], out[n * 5 + 1:]


def combine_semantic_and_instance_outputs(instance_results, semantic_results, overlap_threshold, stuff_area_thresh,
                                          instances_score_thresh) -> Tuple[torch.Tensor, List[Dict]]:
    """panoptic_fpn.py:184-269 -- `instance_results`: anything with `scores`, `pred_classes` and `pred_masks` (R, H, W)
    bool / uint8; `semantic_results` the (H, W) category ids.  -> (panoptic_seg int32 (H, W), segments_info) with the
    reference's dicts: things carry id / isthing / score / category_id / instance_id, stuff id / isthing / category_id /
    area.  Equal scores are ranked by lower index; labels of 256 and above get no segment."""
    scores = instance_results.scores
    seg, out, n_rows = _combine(scores, instance_results.pred_classes, semantic_results, overlap_threshold,
                                stuff_area_thresh, instances_score_thresh, instance_results.pred_masks, None, None, 0.5,
                                MAX_CLASSES)
    # the one host transfer: the rows, the count behind them and the scores' bits
    host = torch.cat([out[:n_rows * 5 + 1], scores.detach().double().view(torch.int64)]).cpu()
    rows = host[:n_rows * 5].view(n_rows, 5)[:int(host[n_rows * 5])].tolist()
    score_of = host[n_rows * 5 + 1:].view(torch.float64).tolist()
    info = []
    for sid, isthing, category, inst, area in rows:
        if isthing:
            info.append({"id": sid, "isthing": True, "score": score_of[inst], "category_id": category, "instance_id": inst})
        else:
            info.append({"id": sid, "isthing": False, "category_id": category, "area": area})
    return seg, info
