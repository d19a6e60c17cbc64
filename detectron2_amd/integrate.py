"""Level-1 integration as ONE call: bind an imported `detectron2` package's hot-path entry points to
this library -- the layer modules AND the fused callers either side of them -- without touching a model's code:

    import detectron2, detectron2_amd.integrate as integrate
    patched = integrate.patch(detectron2)          # before build_model(cfg) (classes are swapped), or with models=[m]
    ...
    patched.undo()                                 # (also a context manager)

What is bound, and what it replaces (reference file:line under the Detectron2 tree):

  names re-exported by `detectron2.layers` (layers/__init__.py:2-16)      -> detectron2_amd.layers.*
      ROIAlign, roi_align, ROIAlignRotated, roi_align_rotated, DeformConv, ModulatedDeformConv, deform_conv,
      modulated_deform_conv, nms, batched_nms, nms_rotated, batched_nms_rotated, paste_masks_in_image,
      pairwise_iou_rotated
  structures/boxes.py:312-377 pairwise_iou / pairwise_ioa                  -> the fused IoU kernels; under a `Matcher`
      the matrix is never written: pairwise_iou returns a LAZY matrix, `Matcher.__call__` (modeling/matcher.py:61-127)
      recognises it and runs Matcher.match_boxes (rpn.py:331-353, roi_heads.py:257-295 read nothing else of it);
      any other use of the lazy object materialises the matrix
  modeling/poolers.py:112-263 ROIPooler                                    -> the fused multi-level pooler (class for models
      built afterwards; instances inside `models` are converted in place and restored by undo()); the box head's and the
      mask head's poolers of one iteration chain into the PAIRED backward by themselves
  proposal_generator/rpn.py:482-512 RPN.predict_proposals                  -> find_top_rpn_proposals_fused (decode + per-level
      top-k + clip + NMS + top-k for the batch, one host read)
  roi_heads/fast_rcnn.py:44-170 fast_rcnn_inference                        -> fast_rcnn_inference_fused
  roi_heads/mask_head.py:33-158 mask_rcnn_loss / mask_rcnn_inference       -> the device-side glue (bit masks cropped for the
      whole batch in one launch)
  roi_heads/keypoint_head.py:40-132 keypoint_rcnn_loss / keypoint_rcnn_inference -> the fused loss (targets in the kernel, no
      host read) and the one-launch heatmap decode; rebound in that module only
  meta_arch/retinanet.py:160-210 RetinaNet.losses, proposal_generator/rpn.py:366-429 RPN.losses -> the fused dense-anchor
      losses (one forward and one backward launch for all images and levels, no host read; smooth_l1 / giou, 4-column
      boxes, device tensors -- anything else stays the reference's method)
  meta_arch/semantic_seg.py:255-267 SemSegFPNHead.losses                   -> the fused upsampling + cross-entropy
      (`sem_seg_loss`: no full-res logits; common_stride 2 / 4 / 8, <= 256 classes, device tensors -- anything else stays
      the reference's method).  The inference side, `sem_seg_labels`, replaces three lines of the caller: INTEGRATION.md
  meta_arch/panoptic_fpn.py:184-269 combine_semantic_and_instance_outputs   -> the fused merge of things and stuff (four
      launches and one host transfer for the host loop's ~350 reads; device tensors, <= 128 detections, bool / uint8
      masks -- anything else stays the reference's function)
  roi_heads/fast_rcnn.py:307-352 FastRCNNOutputLayers.losses               -> the fused box-head loss (`fast_rcnn_losses`: no
      argmax / nonzero / gather, no host read), ONLY when `only` names "box_loss": it is not part of the default set

NOT bound: the samplers (`subsample_labels`, sampling.py:9-54, is defined by torch's RNG; this library's sampler is
defined by explicit keys -- the same distribution, other draws: a bound sampler changes WHICH rows are sampled, so it is
offered separately, `samplers=True`).

Product glue only: no CPU path, no fallback -- a tensor that is not on a HIP device raises as everywhere in this package.
"""
import sys
from typing import Iterable, List, Optional

import torch

__all__ = ["patch", "Patched", "LazyIoU"]


class LazyIoU:
    """`pairwise_iou(gt, boxes)` not yet evaluated.  `Matcher.__call__` consumes it without the matrix; anything else
    (`.max(...)`, indexing, torch functions through `.tensor()`) evaluates it once and forwards."""

    def __init__(self, boxes1, boxes2):
        self.boxes1, self.boxes2 = boxes1, boxes2
        self._m = None

    def tensor(self):
        if self._m is None:
            from .structures import Boxes, pairwise_iou

            self._m = pairwise_iou(Boxes(self.boxes1), Boxes(self.boxes2))
        return self._m

    def __getattr__(self, name):  # (only names the object does not have: everything of the matrix)
        return getattr(self.tensor(), name)

    def __getitem__(self, idx):
        return self.tensor()[idx]

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        un = lambda a: a.tensor() if isinstance(a, LazyIoU) else a
        return func(*[un(a) for a in args], **{k: un(v) for k, v in (kwargs or {}).items()})


class Patched:
    """Handle of one `patch()`: `.undo()` restores every binding (names, methods, converted pooler instances)."""

    def __init__(self):
        self._names, self._attrs, self._mods = [], [], []

    def _set(self, obj, name, new):
        self._attrs.append((obj, name, obj.__dict__.get(name, getattr(obj, name))))
        setattr(obj, name, new)

    def undo(self):
        for obj, name, old in reversed(self._attrs):
            setattr(obj, name, old)
        for parent, name, old in reversed(self._mods):
            setattr(parent, name, old)
        self._attrs, self._mods = [], []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.undo()
        return False


def _rebind_everywhere(h: Patched, pkg: str, name: str, orig, new):
    """Every module of the package that bound `name` to `orig` at import time (from ... import name) gets `new`."""
    for mod in list(sys.modules.values()):
        if mod is None or not getattr(mod, "__name__", "").startswith(pkg):
            continue
        if mod.__dict__.get(name) is orig:
            h._set(mod, name, new)


def _convert_pooler(ref):
    """The reference's ROIPooler instance -> this library's, same configuration (poolers.py:112-204)."""
    from .modeling.poolers import ROIPooler

    lp = ref.level_poolers[0]
    kind = type(lp).__name__
    if kind == "ROIAlign":
        ptype = "ROIAlignV2" if lp.aligned else "ROIAlign"
    elif kind == "ROIAlignRotated":
        ptype = "ROIAlignRotated"
    else:
        return None  # (ROIPool: torchvision's max pooling, on no BASELINE config)
    return ROIPooler(tuple(ref.output_size), [float(p.spatial_scale) for p in ref.level_poolers], int(lp.sampling_ratio),
                     ptype, canonical_box_size=ref.canonical_box_size, canonical_level=ref.canonical_level)


def patch(detectron2=None, models: Iterable = (), layers: bool = True, fused: bool = True, samplers: bool = False,
          only: Optional[Iterable[str]] = None) -> Patched:
    """Bind `detectron2` (default: the imported package) to this library; see the module docstring.  `models`: already
    built models whose ROIPooler instances are converted in place.  `only`: a subset of the fused bindings
    {"matcher", "pooler", "rpn", "box_inference", "mask_head", "keypoint_head", "sem_seg", "panoptic", "dense", "dense_loss"} (default: all of them), and "box_loss", which is bound
    only when named here."""
    want = lambda k: only is None or k in set(only)
    if detectron2 is None:
        import detectron2  # noqa: F811
    pkg = detectron2.__name__
    import importlib

    imp = lambda n: importlib.import_module(pkg + "." + n)
    from . import layers as L
    from . import modeling as M
    from . import structures as S

    h = Patched()
    d2_boxes = imp("structures.boxes")
    D2Boxes = d2_boxes.Boxes
    if layers:
        d2l = imp("layers")
        for name in ("ROIAlign", "roi_align", "ROIAlignRotated", "roi_align_rotated", "DeformConv", "ModulatedDeformConv",
                     "deform_conv", "modulated_deform_conv", "nms", "batched_nms", "nms_rotated", "batched_nms_rotated",
                     "pairwise_iou_rotated"):
            if hasattr(d2l, name) and hasattr(L, name):
                _rebind_everywhere(h, pkg, name, getattr(d2l, name), getattr(L, name))

        def paste_masks_in_image(masks, boxes, image_shape, threshold: float = 0.5):
            return L.paste_masks_in_image(masks, getattr(boxes, "tensor", boxes), image_shape, threshold)

        _rebind_everywhere(h, pkg, "paste_masks_in_image", imp("layers.mask_ops").paste_masks_in_image, paste_masks_in_image)

        def pairwise_ioa(b1, b2):
            return S.pairwise_ioa(S.Boxes(b1.tensor), S.Boxes(b2.tensor))

        _rebind_everywhere(h, pkg, "pairwise_ioa", d2_boxes.pairwise_ioa, pairwise_ioa)
        if not fused:
            def pairwise_iou(b1, b2):
                return S.pairwise_iou(S.Boxes(b1.tensor), S.Boxes(b2.tensor))

            _rebind_everywhere(h, pkg, "pairwise_iou", d2_boxes.pairwise_iou, pairwise_iou)
    if not fused:
        return h

    # ---- IoU + Matcher without the matrix
    if not want("matcher"):
        def pairwise_iou(b1, b2):
            return S.pairwise_iou(S.Boxes(b1.tensor), S.Boxes(b2.tensor))

        if layers:
            _rebind_everywhere(h, pkg, "pairwise_iou", d2_boxes.pairwise_iou, pairwise_iou)

    def pairwise_iou_lazy(b1, b2):
        return LazyIoU(b1.tensor, b2.tensor)

    if want("matcher"):
        _rebind_everywhere(h, pkg, "pairwise_iou", d2_boxes.pairwise_iou, pairwise_iou_lazy)
    d2_matcher = imp("modeling.matcher").Matcher
    ref_call = d2_matcher.__call__

    def matcher_call(self, match_quality_matrix):
        if isinstance(match_quality_matrix, LazyIoU):
            mine = getattr(self, "_d2amd", None)
            if mine is None:
                mine = M.Matcher(list(self.thresholds[1:-1]), list(self.labels), self.allow_low_quality_matches)
                self._d2amd = mine
            q = match_quality_matrix
            if q.boxes1.shape[0] == 0:  # (matcher.py:79-88: no ground truth -> everything unmatched; no kernel)
                return ref_call(self, q.tensor())
            return mine.match_boxes(q.boxes1, q.boxes2)
        return ref_call(self, match_quality_matrix)

    if want("matcher"):
        h._set(d2_matcher, "__call__", matcher_call)

    # ---- ROIPooler: the class (models built from now on) and the instances of `models`
    d2_poolers = imp("modeling.poolers")
    ref_pooler_cls = d2_poolers.ROIPooler
    if want("pooler"):
        _rebind_everywhere(h, pkg, "ROIPooler", ref_pooler_cls, M.ROIPooler)
    for model in (models if want("pooler") else ()):
        for parent in model.modules():
            for name, child in list(parent.named_children()):
                if isinstance(child, ref_pooler_cls):
                    mine = _convert_pooler(child)
                    if mine is not None:
                        mine.to(next(iter(model.parameters())).device)
                        h._mods.append((parent, name, child))
                        setattr(parent, name, mine)

    # ---- RPN: decode + selection + NMS for the batch
    Instances = imp("structures").Instances
    rpn = imp("modeling.proposal_generator.rpn")
    ref_predict = rpn.RPN.predict_proposals

    def predict_proposals(self, anchors, pred_objectness_logits, pred_anchor_deltas, image_sizes):
        tr = self.box2box_transform
        if (type(tr).__name__ != "Box2BoxTransform" or len(anchors) == 0 or anchors[0].tensor.shape[-1] != 4
                or not pred_objectness_logits[0].is_cuda):
            return ref_predict(self, anchors, pred_objectness_logits, pred_anchor_deltas, image_sizes)
        with torch.no_grad():
            props = M.find_top_rpn_proposals_fused(
                [a.tensor for a in anchors], [x.detach() for x in pred_objectness_logits],
                [x.detach() for x in pred_anchor_deltas], [tuple(s) for s in image_sizes], self.nms_thresh,
                self.pre_nms_topk[self.training], self.post_nms_topk[self.training], self.min_box_size, self.training,
                weights=tuple(tr.weights), scale_clamp=tr.scale_clamp)
        out = []
        for p in props:
            res = Instances(tuple(p.image_size))
            res.proposal_boxes = D2Boxes(p.proposal_boxes.tensor)
            res.objectness_logits = p.objectness_logits
            out.append(res)
        return out

    if want("rpn"):
        h._set(rpn.RPN, "predict_proposals", predict_proposals)

    # ---- box head inference
    fr = imp("modeling.roi_heads.fast_rcnn")

    def fast_rcnn_inference(boxes, scores, image_shapes, score_thresh, nms_thresh, topk_per_image):
        dets, rows = M.fast_rcnn_inference_fused(boxes, scores, image_shapes, score_thresh, nms_thresh, topk_per_image)
        out = []
        for d in dets:
            res = Instances(tuple(d.image_size))
            res.pred_boxes = D2Boxes(d.pred_boxes.tensor)
            res.scores = d.scores
            res.pred_classes = d.pred_classes
            out.append(res)
        return out, rows

    if want("box_inference"):
        _rebind_everywhere(h, pkg, "fast_rcnn_inference", fr.fast_rcnn_inference, fast_rcnn_inference)

    # ---- mask head glue
    mh = imp("modeling.roi_heads.mask_head")
    d2_masks = imp("structures.masks")

    class _Row:  # (what mask_rcnn_loss reads of an Instances; reference BitMasks -> this library's, same storage)
        def __init__(self, inst):
            self._n = len(inst)
            self.gt_classes, self.proposal_boxes = inst.gt_classes, inst.proposal_boxes
            gm = inst.gt_masks
            self.gt_masks = S.BitMasks(gm.tensor) if isinstance(gm, d2_masks.BitMasks) and gm.tensor.is_cuda else gm

        def __len__(self):
            return self._n

    def mask_rcnn_loss(pred_mask_logits, instances, vis_period: int = 0):
        if vis_period > 0:  # (the reference's image logging path: unchanged)
            return ref_loss(pred_mask_logits, instances, vis_period)
        return M.mask_rcnn_loss(pred_mask_logits, [_Row(i) for i in instances])

    ref_loss = mh.mask_rcnn_loss
    if want("mask_head"):
        _rebind_everywhere(h, pkg, "mask_rcnn_loss", ref_loss, mask_rcnn_loss)
        _rebind_everywhere(h, pkg, "mask_rcnn_inference", mh.mask_rcnn_inference, M.mask_rcnn_inference)

    # ---- keypoint head glue.  Bound in keypoint_head's own namespace ONLY (BaseKeypointRCNNHead.forward,
    # keypoint_head.py:183-205, looks the two names up there): a package-wide rebind would also replace them in modules
    # that re-exported the originals for other callers.
    try:
        kh = imp("modeling.roi_heads.keypoint_head")
    except ImportError:  # (a trimmed package without the keypoint head)
        kh = None
    if kh is not None and want("keypoint_head"):
        ref_kp_loss, ref_kp_inference = kh.keypoint_rcnn_loss, kh.keypoint_rcnn_inference

        def keypoint_rcnn_loss(pred_keypoint_logits, instances, normalizer):
            # CPU tensors, and the batch without instances (whose kpts_num_skipped_batches log stays the reference's)
            if not pred_keypoint_logits.is_cuda or all(len(i) == 0 for i in instances):
                return ref_kp_loss(pred_keypoint_logits, instances, normalizer)
            return M.keypoint_rcnn_loss(pred_keypoint_logits, instances, normalizer)

        def keypoint_rcnn_inference(pred_keypoint_logits, pred_instances):
            if not pred_keypoint_logits.is_cuda:
                return ref_kp_inference(pred_keypoint_logits, pred_instances)
            return M.keypoint_rcnn_inference(pred_keypoint_logits, pred_instances)

        h._set(kh, "keypoint_rcnn_loss", keypoint_rcnn_loss)
        h._set(kh, "keypoint_rcnn_inference", keypoint_rcnn_inference)

    # ---- semantic-segmentation head: SemSegFPNHead.losses (semantic_seg.py:255-267), upsampling + cross-entropy fused
    try:
        ss = imp("modeling.meta_arch.semantic_seg")
    except ImportError:  # (a trimmed package without the semantic head)
        ss = None
    if ss is not None and want("sem_seg"):
        ref_sem_seg_losses = ss.SemSegFPNHead.losses

        def sem_seg_losses(self, predictions, targets):
            from .modeling.sem_seg import MAX_CLASSES, SCALES

            if not predictions.is_cuda or self.common_stride not in SCALES or predictions.shape[1] > MAX_CLASSES:
                return ref_sem_seg_losses(self, predictions, targets)
            return {"loss_sem_seg": M.sem_seg_loss(predictions, targets, common_stride=self.common_stride,
                                                   ignore_value=self.ignore_value, loss_weight=self.loss_weight)}

        h._set(ss.SemSegFPNHead, "losses", sem_seg_losses)

    # ---- Panoptic FPN merge: combine_semantic_and_instance_outputs (panoptic_fpn.py:184-269), looked up in its module by
    # PanopticFPN.forward_inference at every call
    try:
        pf = imp("modeling.meta_arch.panoptic_fpn")
    except ImportError:  # (a trimmed package without Panoptic FPN)
        pf = None
    if pf is not None and want("panoptic"):
        ref_combine = pf.combine_semantic_and_instance_outputs

        def combine_semantic_and_instance_outputs(instance_results, semantic_results, overlap_threshold, stuff_area_thresh,
                                                  instances_score_thresh):
            from .modeling.panoptic import MAX_DETECTIONS

            masks = instance_results.pred_masks
            if (not semantic_results.is_cuda or not masks.is_cuda or len(instance_results.scores) > MAX_DETECTIONS
                    or masks.dtype not in (torch.bool, torch.uint8)):
                return ref_combine(instance_results, semantic_results, overlap_threshold, stuff_area_thresh,
                                   instances_score_thresh)
            return M.combine_semantic_and_instance_outputs(instance_results, semantic_results, overlap_threshold,
                                                           stuff_area_thresh, instances_score_thresh)

        h._set(pf, "combine_semantic_and_instance_outputs", combine_semantic_and_instance_outputs)

    # ---- RetinaNet inference: per-level threshold + top-k + decode and the per-class NMS of the batch in one device
    # pipeline (retinanet.py:257-309, dense_detector.py:186-260: a Python loop over images x levels with a nonzero / topk /
    # index chain and one batched_nms per image)
    try:
        rn = imp("modeling.meta_arch.retinanet")
    except ImportError:  # (a trimmed package without the dense detectors)
        rn = None
    if rn is not None and want("dense"):
        ref_forward_inference = rn.RetinaNet.forward_inference

        def forward_inference(self, images, features, predictions):
            tr = self.box2box_transform
            if type(tr).__name__ != "Box2BoxTransform" or len(features) == 0 or not features[0].is_cuda:
                return ref_forward_inference(self, images, features, predictions)
            pred_logits, pred_anchor_deltas = self._transpose_dense_predictions(predictions, [self.num_classes, 4])
            anchors = self.anchor_generator(features)
            dets = M.dense_detector_inference_fused(
                [a.tensor for a in anchors], pred_logits, pred_anchor_deltas, [tuple(sz) for sz in images.image_sizes],
                self.test_score_thresh, self.test_topk_candidates, self.test_nms_thresh, self.max_detections_per_image,
                weights=tuple(tr.weights), scale_clamp=tr.scale_clamp)
            out = []
            for d in dets:
                res = Instances(tuple(d.image_size))
                res.pred_boxes = D2Boxes(d.pred_boxes.tensor)
                res.scores = d.scores
                res.pred_classes = d.pred_classes
                out.append(res)
            return out

        h._set(rn.RetinaNet, "forward_inference", forward_inference)

    # ---- dense-anchor training losses: RPN.losses and RetinaNet.losses
    def _fused_loss_ok(self, anchors, logits):
        return (type(self.box2box_transform).__name__ == "Box2BoxTransform" and self.box_reg_loss_type in ("smooth_l1", "giou")
                and len(anchors) > 0 and anchors[0].tensor.shape[-1] == 4 and len(logits) > 0 and logits[0].is_cuda)

    if want("dense_loss"):
        ref_rpn_losses = rpn.RPN.losses

        def rpn_losses(self, anchors, pred_objectness_logits, gt_labels, pred_anchor_deltas, gt_boxes):
            """RPN.losses on the fused kernels.  The event-storage scalars rpn/num_pos_anchors and rpn/num_neg_anchors are
            NOT logged: `put_scalar` takes a host float, and the counts stay on the device here."""
            if not _fused_loss_ok(self, anchors, pred_objectness_logits):
                return ref_rpn_losses(self, anchors, pred_objectness_logits, gt_labels, pred_anchor_deltas, gt_boxes)
            tr = self.box2box_transform
            return M.rpn_losses([a.tensor for a in anchors], pred_objectness_logits, gt_labels, pred_anchor_deltas, gt_boxes,
                                batch_size_per_image=self.batch_size_per_image, box_reg_loss_type=self.box_reg_loss_type,
                                smooth_l1_beta=self.smooth_l1_beta, box2box_weights=tuple(tr.weights),
                                loss_weight=self.loss_weight, scale_clamp=tr.scale_clamp)

        h._set(rpn.RPN, "losses", rpn_losses)
    if rn is not None and want("dense_loss"):
        ref_retinanet_losses = rn.RetinaNet.losses

        def retinanet_losses(self, anchors, pred_logits, gt_labels, pred_anchor_deltas, gt_boxes):
            """RetinaNet.losses on the fused kernels.  The EMA of the foreground count lives in a 1-element device tensor
            (`_d2amd_loss_normalizer`, started from `loss_normalizer` or 100) and the event-storage scalar
            num_pos_anchors is NOT logged: both would need the count on the host."""
            if not _fused_loss_ok(self, anchors, pred_logits):
                return ref_retinanet_losses(self, anchors, pred_logits, gt_labels, pred_anchor_deltas, gt_boxes)
            tr = self.box2box_transform
            cls, box, stats = M.dense_anchor_losses(
                [a.tensor for a in anchors], pred_logits, pred_anchor_deltas, gt_labels, gt_boxes, label_mode="class",
                alpha=self.focal_loss_alpha, gamma=self.focal_loss_gamma, box_reg_loss_type=self.box_reg_loss_type,
                smooth_l1_beta=self.smooth_l1_beta, weights=tuple(tr.weights), scale_clamp=tr.scale_clamp)
            state = self.__dict__.get("_d2amd_loss_normalizer")
            if state is None or state.device != cls.device:
                state = torch.full((1,), float(getattr(self, "loss_normalizer", 100)), device=cls.device)
                self.__dict__["_d2amd_loss_normalizer"] = state
            normalizer = M.ema_normalizer_(state, stats).reshape(())
            return {"loss_cls": cls / normalizer, "loss_box_reg": box / normalizer}

        h._set(rn.RetinaNet, "losses", retinanet_losses)

    # ---- box head training loss: FastRCNNOutputLayers.losses.  Bound only when NAMED in `only`.
    if only is not None and "box_loss" in set(only):
        ref_box_losses = fr.FastRCNNOutputLayers.losses

        def box_losses(self, predictions, proposals):
            """FastRCNNOutputLayers.losses on the fused kernels.  The event-storage scalars fast_rcnn/cls_accuracy,
            fast_rcnn/fg_cls_accuracy and fast_rcnn/false_negative are NOT logged: `put_scalar` takes host floats, and
            the five counts they are made of stay on the device, in `self._d2amd_box_loss_stats` (int64 [5]: rows,
            foreground rows, accurate, accurate foreground, foreground predicted as background)."""
            scores, proposal_deltas = predictions
            if (type(self.box2box_transform).__name__ != "Box2BoxTransform" or not scores.is_cuda or len(proposals) == 0
                    or self.box_reg_loss_type not in ("smooth_l1", "giou")
                    or proposals[0].proposal_boxes.tensor.shape[-1] != 4):
                return ref_box_losses(self, predictions, proposals)
            gt_classes = torch.cat([p.gt_classes for p in proposals], dim=0)
            proposal_boxes = torch.cat([p.proposal_boxes.tensor for p in proposals], dim=0)
            gt_boxes = torch.cat([(p.gt_boxes if p.has("gt_boxes") else p.proposal_boxes).tensor for p in proposals], dim=0)
            class_weight = None
            if self.use_sigmoid_ce and getattr(self, "use_fed_loss", False):
                k = scores.shape[1] - 1
                keep = self.get_fed_loss_classes(gt_classes, num_fed_loss_classes=self.fed_loss_num_classes, num_classes=k,
                                                 weight=self.fed_loss_cls_weights)
                mask = keep.new_zeros(k + 1)
                mask[keep] = 1
                class_weight = mask[:k].float()
            tr = self.box2box_transform
            losses, stats = M.fast_rcnn_losses_with_stats(
                scores, proposal_deltas, gt_classes, proposal_boxes, gt_boxes, box_reg_loss_type=self.box_reg_loss_type,
                smooth_l1_beta=self.smooth_l1_beta, box2box_weights=tuple(tr.weights), scale_clamp=tr.scale_clamp,
                loss_weight=self.loss_weight, use_sigmoid_ce=self.use_sigmoid_ce, class_weight=class_weight)
            self.__dict__["_d2amd_box_loss_stats"] = stats
            return losses

        h._set(fr.FastRCNNOutputLayers, "losses", box_losses)

    if samplers:
        smp = imp("modeling.sampling")

        def subsample_labels(labels, num_samples, positive_fraction, bg_label):
            return M.subsample_labels(labels, num_samples, positive_fraction, bg_label)

        _rebind_everywhere(h, pkg, "subsample_labels", smp.subsample_labels, subsample_labels)
    return h
