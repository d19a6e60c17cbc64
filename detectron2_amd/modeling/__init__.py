"""Hot-path callers mirrored from `detectron2.modeling` (only what SURVEY.md section 8 lists)."""
from .box_loss import fast_rcnn_losses, fast_rcnn_losses_with_stats
from .dense_detector import Detections, dense_detector_inference_fused, dense_select_predictions
from .dense_loss import (DENSE_LOSS_TILE, dense_anchor_losses, ema_normalizer_, retinanet_label_anchors, retinanet_losses,
                         rpn_losses)
from .fcos import FCOS_GT_CHUNK, fcos_label_anchors, fcos_losses, fcos_losses_from_gt
from .fast_rcnn import DeviceDetections, fast_rcnn_inference_device, fast_rcnn_inference_fused, fast_rcnn_predict
from .keypoint_head import keypoint_rcnn_inference, keypoint_rcnn_loss, keypoint_rcnn_loss_from_targets
from .mask_head import mask_rcnn_inference, mask_rcnn_loss, mask_rcnn_loss_from_targets
from .matcher import Matcher
from .rrpn_loss import MATCH_ROTATED_GT_CHUNK, MATCH_ROTATED_STRIP, rrpn_label_anchors, rrpn_losses
from .proposal_utils import DeviceProposals, Proposals, find_top_rpn_proposals_fused, rpn_select_proposals
from .poolers import ROIPooler, assign_boxes_to_levels, convert_boxes_to_pooler_format, pool_pair, pool_pair_rois, PairBackwardPlan
from .panoptic import combine_semantic_and_instance_outputs, panoptic_combine_device
from .sem_seg import sem_seg_labels, sem_seg_loss, sem_seg_loss_with_stats
from .sampling import (DeviceKeyGenerator, label_and_sample_proposals_fixed, subsample_anchor_labels_, subsample_labels,
                       subsample_labels_batch)

__all__ = ["Detections", "DeviceDetections", "fast_rcnn_inference_device", "fast_rcnn_inference_fused", "fast_rcnn_predict", "dense_detector_inference_fused", "dense_select_predictions", "fast_rcnn_losses", "fast_rcnn_losses_with_stats", "dense_anchor_losses", "retinanet_losses", "rpn_losses", "retinanet_label_anchors", "ema_normalizer_", "DENSE_LOSS_TILE", "keypoint_rcnn_loss", "keypoint_rcnn_inference", "keypoint_rcnn_loss_from_targets", "mask_rcnn_loss", "mask_rcnn_inference", "mask_rcnn_loss_from_targets", "Matcher", "Proposals", "DeviceProposals", "find_top_rpn_proposals_fused", "rpn_select_proposals", "ROIPooler", "pool_pair", "pool_pair_rois", "PairBackwardPlan", "assign_boxes_to_levels", "convert_boxes_to_pooler_format", "subsample_labels", "subsample_labels_batch", "subsample_anchor_labels_", "DeviceKeyGenerator",
           "label_and_sample_proposals_fixed", "sem_seg_loss", "sem_seg_loss_with_stats", "sem_seg_labels",
           "combine_semantic_and_instance_outputs", "panoptic_combine_device", "fcos_label_anchors", "fcos_losses",
           "fcos_losses_from_gt", "FCOS_GT_CHUNK", "rrpn_losses", "rrpn_label_anchors", "MATCH_ROTATED_STRIP",
           "MATCH_ROTATED_GT_CHUNK"]
