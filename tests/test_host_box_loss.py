"""CPU-side checks of the box-head loss entries (include/d2amd.h): argument errors before any launch, and the Python
surface refusing CPU tensors and the box losses the kernel does not have.  No GPU compute."""
import ctypes

import pytest
import torch

from detectron2_amd import _C, modeling

R, K = 8, 3
WTS = (ctypes.c_float * 4)(10, 10, 5, 5)


@pytest.fixture(scope="module")
def lib():
    from detectron2_amd import build

    build.build()
    return _C.lib()


def _args(host, **kw):
    """Arguments of d2amd_fast_rcnn_loss_forward: host buffers stand in for the device's (nothing may be launched)."""
    buf = _C.ptr(host)
    a = dict(scores=buf, deltas=buf, gt_classes=buf, boxes=buf, gt_boxes=buf, gt_index=None, gt_offsets=None, R=R, K=K,
             delta_cols=4 * K, S=0, N=0, G=R, dtype=_C.BF16, cls=0, class_weight=None, box=0, beta=0.0, weights=WTS,
             clamp=4.0, loss=buf, stats=buf, ws=buf, ws_bytes=host.numel(), stream=None)
    assert not set(kw) - set(a)
    a.update(kw)
    return list(a.values())


def test_symbols_and_workspace(lib):
    for name in ("d2amd_fast_rcnn_loss_workspace_bytes", "d2amd_fast_rcnn_loss_forward", "d2amd_fast_rcnn_loss_backward"):
        assert hasattr(lib, name) and name in _C.exported_symbols()
    assert lib.d2amd_fast_rcnn_loss_workspace_bytes(1024) > lib.d2amd_fast_rcnn_loss_workspace_bytes(512) > 0


@pytest.mark.parametrize("bad", [dict(scores=None), dict(gt_classes=None), dict(loss=None), dict(K=0), dict(delta_cols=8),
                                 dict(delta_cols=4 * K + 4), dict(dtype=7), dict(cls=2), dict(box=2), dict(ws_bytes=-1),
                                 dict(ws=None), dict(weights=None)])
def test_bad_arguments_are_einval_before_any_launch(lib, bad):
    ws = torch.zeros(lib.d2amd_fast_rcnn_loss_workspace_bytes(R), dtype=torch.uint8)
    if bad.get("ws_bytes") == -1:
        bad = dict(ws_bytes=ws.numel() - 1)
    fwd = _args(ws, **bad)
    assert lib.d2amd_fast_rcnn_loss_forward(*fwd) == -1 and lib.d2amd_last_error()
    if "loss" not in bad:  # the backward: the same inputs, two upstream gradients, the forward's workspace, two outputs
        buf = _C.ptr(ws)
        bwd = fwd[:7] + [buf, buf] + fwd[7:20] + [fwd[22], fwd[23], buf, buf, None]
        assert lib.d2amd_fast_rcnn_loss_backward(*bwd) == -1 and lib.d2amd_last_error()
    assert lib.d2amd_fast_rcnn_loss_forward(*_args(ws, R=0, scores=None, ws=None, ws_bytes=0)) == 0  # nothing to launch


def test_python_surface_refuses_cpu_tensors_and_missing_box_losses():
    scores, deltas = torch.zeros(R, K + 1), torch.zeros(R, 4 * K)
    classes, boxes = torch.zeros(R, dtype=torch.int64), torch.tensor([[0.0, 0, 10, 10]] * R)
    with pytest.raises(NotImplementedError):
        modeling.fast_rcnn_losses(scores, deltas, classes, boxes, boxes)
    with pytest.raises(NotImplementedError):
        modeling.fast_rcnn_losses_with_stats(scores, deltas, classes, boxes, boxes, use_sigmoid_ce=True)
    for kind in ("diou", "ciou"):  # refused before anything else is looked at
        with pytest.raises(NotImplementedError, match=kind):
            modeling.fast_rcnn_losses(scores, deltas, classes, boxes, boxes, box_reg_loss_type=kind)
    with pytest.raises(NotImplementedError, match="rotated"):
        modeling.fast_rcnn_losses(scores, deltas, classes, torch.zeros(R, 5), torch.zeros(R, 5))
