"""CPU-side checks of the keypoint-head entries (include/d2amd.h): argument errors before any launch, and the Python
surface refusing CPU tensors (no fallback).  No GPU compute."""
import pytest
import torch

from detectron2_amd import _C, modeling, structures


@pytest.fixture(scope="module")
def lib():
    from detectron2_amd import build

    build.build()
    return _C.lib()


@pytest.mark.parametrize("S", [1, 65])
def test_heatmap_side_outside_range_is_rejected(lib, S):
    calls = [lib.d2amd_keypoints_to_heatmap(None, None, 2, 17, S, None, None, None),
             lib.d2amd_keypoint_rcnn_loss_forward(None, None, None, 2, 17, S, 0, 0.0, None, None, None, 0, None),
             lib.d2amd_keypoint_rcnn_loss_backward(None, None, None, 2, 17, S, 0, 0.0, None, None),
             lib.d2amd_heatmaps_to_keypoints(None, None, 2, 17, S, 0, None, None, None)]
    assert calls == [-1] * 4 and b"heatmap side" in lib.d2amd_last_error()


def test_short_workspace_is_rejected_and_empty_batches_succeed(lib):
    need = lib.d2amd_keypoint_rcnn_loss_workspace_bytes(34)
    assert need > lib.d2amd_keypoint_rcnn_loss_workspace_bytes(17) > 0
    buf = torch.zeros(need, dtype=torch.uint8)
    rc = lib.d2amd_keypoint_rcnn_loss_forward(None, None, None, 2, 17, 56, 0, 0.0, None, None, _C.ptr(buf), need - 1, None)
    assert rc == -1 and b"workspace too small" in lib.d2amd_last_error()
    assert lib.d2amd_keypoint_rcnn_loss_forward(None, None, None, 0, 17, 56, 0, 0.0, None, None, None, 0, None) == 0
    assert lib.d2amd_keypoint_rcnn_loss_backward(None, None, None, 0, 17, 56, 0, 0.0, None, None) == 0
    assert lib.d2amd_heatmaps_to_keypoints(None, None, 0, 17, 56, 0, None, None, None) == 0
    assert lib.d2amd_keypoints_to_heatmap(None, None, 0, 17, 56, None, None, None) == 0


def test_cpu_tensors_are_refused():
    class Inst:
        gt_keypoints = structures.Keypoints(torch.zeros(2, 17, 3))
        proposal_boxes = pred_boxes = structures.Boxes(torch.tensor([[0.0, 0, 10, 10]] * 2))

        def __len__(self):
            return 2

    x = torch.zeros(2, 17, 56, 56)
    with pytest.raises(NotImplementedError):
        modeling.keypoint_rcnn_loss(x, [Inst()], None)
    with pytest.raises(NotImplementedError):
        modeling.keypoint_rcnn_inference(x, [Inst()])
    with pytest.raises(NotImplementedError):
        structures.heatmaps_to_keypoints(x, Inst.pred_boxes.tensor)
    with pytest.raises(NotImplementedError):
        Inst.gt_keypoints.to_heatmap(Inst.pred_boxes.tensor, 56)
    k = structures.Keypoints.cat([Inst.gt_keypoints, Inst.gt_keypoints[0], Inst.gt_keypoints[:1]])
    assert len(k) == 4 and k.device.type == "cpu" and repr(k) == "Keypoints(num_instances=4)"
