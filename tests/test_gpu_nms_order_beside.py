"""NMS from pre-sorted runs that are the categories, n <= 12,288 (the RPN's and the inference chain's configuration):
the score order is merged BESIDE the reduction (nms_reduce_order_kernel) and no longer in front of the mask, which
gets its box records from a streaming kernel (csrc/nms.hip, step 1c).  Every case here is compared, bit for bit,
  * with the CPU oracle (oracle.batched_nms with category = run index), and
  * with the earlier launch sequence (order + records in one launch in front of the mask), which the library still
    runs under D2AMD_NMS_ORDER_FIRST (read per call),
through d2amd_nms_runs (ops._nms_launch) and d2amd_nms_batched_runs (ops.nms_images), runs_are_categories = 1.

d2amd_nms_batched_runs takes ONE run table for the whole batch and rejects an image whose n is not the table's total
(an empty image excepted), so "images of different n in one batch" can only be: empty image + full images whose live
counts differ; that is the batch case below."""
import os

import numpy as np
import pytest
import torch

import oracle
from detectron2_amd.layers import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
SWITCH = "D2AMD_NMS_ORDER_FIRST"


def _split(n, k, g):
    """k run lengths that sum to n: uneven, boundaries off the multiples of 64, empty runs when n < k"""
    if k == 1:
        return (n,)
    cuts = sorted(int(c) for c in torch.randint(0, n + 1, (k - 1,), generator=g))
    cuts = [0] + cuts + [n]
    return tuple(b - a for a, b in zip(cuts[:-1], cuts[1:]))


def _make(seed, lens, rotated=False, parked=0.1, ties=True, park_tail=(), park_all=()):
    """rows = runs of the given lengths in descending score order (few distinct scores when `ties`: equal scores inside
    and across runs), some rows parked at -inf (zero boxes) anywhere; runs in park_tail end in a block of parked rows,
    runs in park_all are parked entirely"""
    g = torch.Generator().manual_seed(seed)
    n = sum(lens)
    extent = 60.0 + 9.0 * float(np.sqrt(n))
    c = torch.rand(n, 2, generator=g) * extent
    wh = 20 + torch.rand(n, 2, generator=g) * 100
    if rotated:
        boxes = torch.cat([c, wh, torch.rand(n, 1, generator=g) * 180 - 90], 1)
    else:
        boxes = torch.cat([c - wh / 2, c + wh / 2], 1)
    parts = []
    for q, ln in enumerate(lens):
        s = torch.randint(0, max(ln // 3, 2), (ln,), generator=g).float() / 7 if ties else torch.randn(ln, generator=g)
        s = torch.sort(s, descending=True).values
        if q in park_tail:
            s[ln - ln // 4:] = float("-inf")
        if q in park_all:
            s[:] = float("-inf")
        parts.append(s)
    scores = torch.cat(parts)
    scores[torch.rand(n, generator=g) < parked] = float("-inf")
    boxes[scores == float("-inf")] = 0
    off = np.concatenate([[0], np.cumsum(lens)]).astype(int).tolist()
    cat = torch.repeat_interleave(torch.arange(len(lens)), torch.tensor(lens))
    return boxes, scores, cat, off


def _launch(b, s, off, thr, rotated, order_first=False):
    """d2amd_nms_runs -> (kept indices, result[0:4]) on the host"""
    old = os.environ.pop(SWITCH, None)
    try:
        if order_first:
            os.environ[SWITCH] = "1"
        keep, result, _hold = ops._nms_launch(b.to(DEV), s.to(DEV), None, thr, rotated, runs=(off, True))
        res = result.cpu().tolist()
    finally:
        os.environ.pop(SWITCH, None)
        if old is not None:
            os.environ[SWITCH] = old
    return keep[:res[0]].cpu().numpy(), res


def _expect(b, s, cat, thr, rotated):
    keep = oracle.batched_nms(b.numpy(), s.numpy(), cat.numpy(), thr, rotated)
    return keep, int((s.numpy()[keep] > -np.inf).sum())


def _check(b, s, cat, off, thr=0.7, rotated=False):
    exp, exp_fin = _expect(b, s, cat, thr, rotated)
    new, rnew = _launch(b, s, off, thr, rotated)
    old, rold = _launch(b, s, off, thr, rotated, order_first=True)
    assert rnew == rold, (rnew, rold)
    assert np.array_equal(new, old)
    assert rnew[1] == 0 and rnew[0] == len(exp) and rnew[2] == exp_fin, (rnew, len(exp), exp_fin)
    assert np.array_equal(new, exp)
    return new


@pytest.mark.parametrize("k", [1, 2, 5])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_block_and_workgroup_edges(n, k):
    g = torch.Generator().manual_seed(100 * n + k)
    lens = _split(n, k, g)
    assert sum(lens) == n and len(lens) == k
    b, s, cat, off = _make(n + k, lens)
    _check(b, s, cat, off, 0.7)


@pytest.mark.parametrize("thr", [0.7, 0.5])
@pytest.mark.parametrize("lens", [
    (100, 37, 251, 1, 190),          # run boundaries inside keepbits words
    (0, 300, 130), (300, 0, 130), (300, 130, 0), (0, 0, 7, 0),  # empty first / middle / last run
    (2240, 100), (2241, 100), (30, 2240),  # the reduction's HALF switch: 35 / 36 blocks of one run
])
def test_run_layouts(lens, thr):
    b, s, cat, off = _make(len(lens) * 1000 + lens[0], lens)
    _check(b, s, cat, off, thr)


def test_parked_entries():
    lens = (400, 333, 200, 90)
    b, s, cat, off = _make(5, lens, park_tail=(0, 2), park_all=(1,))
    assert bool((s[400:733] == float("-inf")).all())
    keep = _check(b, s, cat, off)
    assert (s.numpy()[keep] == -np.inf).any()  # parked rows are kept (zero boxes) but not counted in result[2]
    b, s, cat, off = _make(6, lens, park_all=(0, 1, 2, 3))  # nothing live at all
    _check(b, s, cat, off)


def test_equal_scores_across_and_inside_runs():
    lens = (130, 130, 130)
    b, s, cat, off = _make(7, lens, parked=0.0)
    s = torch.cat([torch.sort(torch.tensor([1.0, 0.5, 0.5, 0.25] * 33)[:130], descending=True).values] * 3)
    _check(b, s, cat, off)
    _check(b, torch.full_like(s, 0.5), cat, off)  # one score everywhere: array order


def test_run_that_is_not_in_order():
    lens = (500, 1100, 300)
    b, s, cat, off = _make(8, lens, ties=False, parked=0.0)
    s2 = s.clone()
    s2[[10, 400]] = s2[[400, 10]]
    s2[[1700, 1850]] = s2[[1850, 1700]]  # a second workgroup of the order sees one too
    _, rnew = _launch(b, s2, off, 0.7, False)
    _, rold = _launch(b, s2, off, 0.7, False, order_first=True)
    assert rnew[1] == 4 and rnew[2] == 0 and rnew[3] == 0
    assert rold[1] == 4 and rold[2] == 0
    # through the batched entry the image is redone from scratch
    (keep,) = ops.nms_images([(b.to(DEV), s2.to(DEV), None)], 0.7, runs=(off, True))
    exp, _ = _expect(b, s2, cat, 0.7, False)
    assert np.array_equal(keep.cpu().numpy(), exp)


def test_batch_of_images():
    lens = (700, 1, 350, 64)
    ins = [_make(20, lens), _make(21, lens, parked=0.6), _make(22, lens, park_all=(0, 2))]
    off = ins[0][3]
    empty = (torch.zeros(0, 4), torch.zeros(0), None)
    batch = [(b.to(DEV), s.to(DEV), None) for b, s, _c, _o in ins]
    batch.insert(1, tuple(None if t is None else t.to(DEV) for t in empty))
    keeps, fin, _ = ops.nms_images(batch, 0.7, defer=True, runs=(off, True))(with_finite=True)
    assert len(keeps[1]) == 0 and fin[1] == 0
    for (b, s, cat, _o), k, f in zip(ins, [keeps[0], keeps[2], keeps[3]], [fin[0], fin[2], fin[3]]):
        exp, exp_fin = _expect(b, s, cat, 0.7, False)
        assert np.array_equal(k.cpu().numpy(), exp) and f == exp_fin


def test_non_finite_coordinate_and_degenerate_boxes():
    lens = (150, 100)
    b, s, cat, off = _make(9, lens, parked=0.0)
    b2 = b.clone()
    b2[70, 2] = float("inf")  # one tile takes the literal formula
    b2[200, 0] = float("nan")
    _check(b2, s, cat, off)
    b3 = b.clone()
    b3[5:40:3, 2] = b3[5:40:3, 0]  # zero width
    b3[41:90:4, [0, 2]] = b3[41:90:4, [2, 0]]  # negative width: area = (x2 - x1) * (y2 - y1) < 0
    b3[160:200:5, [1, 3]] = b3[160:200:5, [3, 1]]
    _check(b3, s, cat, off)
    _check(b3, s, cat, off, 0.5)


@pytest.mark.parametrize("n", [65, 1025])
def test_rotated(n):
    g = torch.Generator().manual_seed(n)
    lens = _split(n, 2, g)
    b, s, cat, off = _make(n, lens, rotated=True)
    _check(b, s, cat, off, 0.5, rotated=True)


@pytest.mark.parametrize("arrays", [1, 2, 4])
def test_gather_in_keep_order(arrays):
    lens = (900, 700, 450)
    b, s, cat, off = _make(30 + arrays, lens)
    g = torch.Generator().manual_seed(arrays)
    src = [b, s, cat.to(torch.int64), torch.rand(sum(lens), 2, generator=g)][:arrays]
    src = [t.to(DEV) for t in src]
    done = ops.nms_images([(b.to(DEV), s.to(DEV), None)], 0.7, defer=True, runs=(off, True), gather=[tuple(src)])
    (keep,), (fin,), _ = done(with_finite=True)
    exp, exp_fin = _expect(b, s, cat, 0.7, False)
    assert np.array_equal(keep.cpu().numpy(), exp) and fin == exp_fin
    for a, d in zip(src, done.gathered[0]):
        assert torch.equal(d[:len(keep)], a[keep])


def test_rpn_shape_and_determinism():
    lens = (2000, 2000, 2000, 2000, 819)
    ins = [_make(40 + i, lens) for i in range(2)]
    off = ins[0][3]
    batch = [(b.to(DEV), s.to(DEV), None) for b, s, _c, _o in ins]
    first = ops.nms_images(batch, 0.7, defer=True, runs=(off, True))(with_finite=True)
    again = ops.nms_images(batch, 0.7, defer=True, runs=(off, True))(with_finite=True)
    os.environ[SWITCH] = "1"
    try:
        before = ops.nms_images(batch, 0.7, defer=True, runs=(off, True))(with_finite=True)
    finally:
        os.environ.pop(SWITCH, None)
    for (b, s, cat, _o), k, f, k2, f2, k3, f3 in zip(ins, first[0], first[1], again[0], again[1], before[0], before[1]):
        exp, exp_fin = _expect(b, s, cat, 0.7, False)
        assert np.array_equal(k.cpu().numpy(), exp) and f == exp_fin
        assert torch.equal(k, k2) and f == f2
        assert torch.equal(k, k3) and f == f3
