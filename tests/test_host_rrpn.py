"""Argument errors of the rotated training entries (Matcher.match_boxes_rotated*, rrpn_label_anchors, rrpn_losses and
their C ABI in csrc/matcher_rot.hip, csrc/rrpn_loss.hip) that are raised on the host before any launch.  No GPU."""
import ctypes

import pytest
import torch

from detectron2_amd import _C
from detectron2_amd.modeling import Matcher, rrpn_label_anchors, rrpn_losses

BUF = ctypes.create_string_buffer(256)
P = ctypes.cast(BUF, ctypes.c_void_p)  # a non-null pointer that no rejected call dereferences
PTRS = (ctypes.c_void_p * 2)(P.value, P.value)
INTS = lambda *v: (ctypes.c_int * len(v))(*v)
THR, LAB = (ctypes.c_float * 1)(0.5), (ctypes.c_int8 * 2)(0, 1)
W5 = (ctypes.c_float * 5)(1, 1, 1, 1, 1)


def test_cpu_tensors_are_refused():
    m = Matcher([0.5], [0, 1])
    g, b = torch.zeros(2, 5), torch.zeros(7, 5)
    for call in (lambda: m.match_boxes_rotated(g, b), lambda: m.match_boxes_rotated_batch([g, g], b),
                 lambda: rrpn_label_anchors([b], [g], m),
                 lambda: rrpn_losses([b], [torch.zeros(1, 7)], torch.zeros(1, 7, dtype=torch.int8), [torch.zeros(1, 7, 5)],
                                     torch.zeros(1, 7, 5), batch_size_per_image=256)):
        with pytest.raises(NotImplementedError, match="no CPU implementation"):
            call()


def _match(gt=PTRS, M=INTS(3, 3), count=2, boxes=P, N=7, thr=THR, T=1, low=1, out=P, ws=P, ws_bytes=1 << 20):
    return _C.lib().d2amd_match_boxes_rotated_batch(gt, M, count, boxes, N, thr, LAB, T, low, out, out, ws, ws_bytes, None)


@pytest.mark.parametrize("kwargs,word", [
    (dict(N=-1), b"negative"), (dict(count=-1), b"negative"), (dict(M=INTS(3, -3)), b"negative"),
    (dict(gt=None), b"null"), (dict(gt=(ctypes.c_void_p * 2)()), b"null"), (dict(boxes=None), b"null"),
    (dict(out=None), b"null"), (dict(ws=None), b"workspace"), (dict(ws_bytes=2 * 64 * 4 + 2 * 7 * 4 - 1), b"workspace"),
    (dict(T=9), b"thresholds"), (dict(thr=(ctypes.c_float * 1)(-0.5)), b"positive"),
])
def test_matcher_c_abi_rejects(kwargs, word):
    assert _match(**kwargs) == -1 and word in _C.lib().d2amd_last_error()


def _loss(backward, ptrs=PTRS, labels=P, N=2, sizes=INTS(300, 1), L=2, dtype=0, beta=0.0, w=W5, out=P, ws_bytes=1 << 20):
    lib = _C.lib()
    if backward:
        return lib.d2amd_rrpn_loss_backward(ptrs, ptrs, ptrs, labels, P, out, out, N, sizes, L, dtype, beta, w, ptrs, ptrs, None)
    return lib.d2amd_rrpn_loss_forward(ptrs, ptrs, ptrs, labels, P, N, sizes, L, dtype, beta, w, out, out, out, P, ws_bytes, None)


@pytest.mark.parametrize("backward", [False, True])
@pytest.mark.parametrize("kwargs,word", [
    (dict(N=-1), b"bad shape"), (dict(sizes=INTS(300, -1)), b"negative"), (dict(L=9, sizes=INTS(*[4] * 9)), b"levels"),
    (dict(sizes=None), b"bad shape"), (dict(dtype=3), b"dtype"), (dict(beta=-1.0), b"beta"), (dict(w=None), b"weights"),
    (dict(w=(ctypes.c_float * 5)(1, 1, 1, 1, 0)), b"positive"), (dict(ptrs=None), b"null"),
    (dict(ptrs=(ctypes.c_void_p * 2)()), b"null level"), (dict(labels=None), b"null"), (dict(out=None), b"null"),
])
def test_loss_c_abi_rejects(backward, kwargs, word):
    assert _loss(backward, **kwargs) == -1 and word in _C.lib().d2amd_last_error()


def test_workspace_sizes_and_empty_calls():
    lib = _C.lib()
    assert _loss(False, ws_bytes=2 * 3 * 16 - 1) == -1 and b"workspace" in lib.d2amd_last_error()
    assert _match(count=0, gt=None, M=None) == 0 and _match(N=0) == 0
    assert lib.d2amd_match_boxes_rotated_batch_workspace_bytes(INTS(65, 3), 2, 7) == 2 * 128 * 4 + 2 * 7 * 4
    assert lib.d2amd_rrpn_loss_workspace_bytes(2, INTS(300, 1), 2) == 2 * 3 * 16  # three tiles per image, 16 B each
    for backward in (False, True):
        assert _loss(backward, N=0, ptrs=None, labels=None, out=None) == 0
        assert _loss(backward, L=0, sizes=None, ptrs=None, labels=None, out=None) == 0
        assert _loss(backward, sizes=INTS(0, 0), ptrs=None, labels=None, out=None) == 0
