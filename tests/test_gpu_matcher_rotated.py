"""The fused rotated matcher (detectron2_amd/csrc/matcher_rot.hip) against the composition it replaces,
`matcher(pairwise_iou_rotated(gt, boxes))` by the existing ops: torch.equal on matches and labels."""
import pytest
import torch

from detectron2_amd.layers import pairwise_iou_rotated
from detectron2_amd.modeling import MATCH_ROTATED_GT_CHUNK, MATCH_ROTATED_STRIP, Matcher

pytestmark = pytest.mark.gpu
DEV = "cuda"
MATCHERS = {"rpn": Matcher([0.3, 0.7], [0, -1, 1], allow_low_quality_matches=True), "roi": Matcher([0.5], [0, 1], False)}
ANGLES = torch.tensor([-90.0, -45.0, 0.0, 30.0, 90.0, 200.0])


def _scene(family, N, M, seed=0):
    """-> (gt [M,5], boxes [N,5]) on the CPU."""
    g = torch.Generator().manual_seed(seed + 1000 * N + M)
    if family == "pile":  # every box within a few pixels of one point: every pair of a strip needs the clip
        mk = lambda n: torch.cat([torch.tensor([400.0, 300.0]) + 6 * torch.rand(n, 2, generator=g),
                                  40 + 20 * torch.rand(n, 2, generator=g), 360 * torch.rand(n, 1, generator=g) - 180], dim=1)
        return mk(M), mk(N)
    # anchors on a grid over an 800 x 1333 image, three sizes x six angles per cell
    cells = -(-N // 18)
    cols = max(1, int((cells * 1333 / 800) ** 0.5))
    ys, xs = torch.meshgrid(torch.arange(-(-cells // cols)), torch.arange(cols), indexing="ij")
    ctr = torch.stack([(xs.flatten() + 0.5) * (1333 / cols), (ys.flatten() + 0.5) * (800 / -(-cells // cols))], dim=1)
    size = torch.tensor([[32.0, 64.0], [128.0, 128.0], [256.0, 96.0]])
    boxes = torch.cat([ctr[:, None, None].expand(-1, 3, 6, 2), size[None, :, None].expand(len(ctr), 3, 6, 2),
                       ANGLES[None, None, :, None].expand(len(ctr), 3, 6, 1)], dim=-1).reshape(-1, 5)[:N].clone()
    pick = boxes[torch.randint(0, N, (M,), generator=g)]
    gt = pick * torch.cat([1 + 0.2 * (torch.rand(M, 4, generator=g) - 0.5), torch.ones(M, 1)], dim=1)
    gt[:, 4] += 20 * (torch.rand(M, generator=g) - 0.5)
    if family == "ties" and M >= 2:
        gt[1] = gt[0]                # two identical ground-truth boxes: the first index wins
        boxes[: min(N, 4)] = gt[0]   # several identical boxes: all get the low-quality label
    if family == "far_gt" and M >= 1:
        gt[M - 1, :2] = 1e5          # overlaps nothing: row maximum 0
    if family == "zero_width":
        boxes[N // 2, 2] = 0.0
        if M >= 1:
            gt[0, 2] = 0.0
    return gt, boxes


@pytest.mark.parametrize("family", ["sparse", "pile", "ties", "far_gt", "zero_width"])
@pytest.mark.parametrize("M", [0, 1, 9, MATCH_ROTATED_GT_CHUNK + 1])
@pytest.mark.parametrize("N", [1, MATCH_ROTATED_STRIP - 1, MATCH_ROTATED_STRIP + 1, 1000])
@pytest.mark.parametrize("which", list(MATCHERS))
def test_equals_the_composition(which, N, M, family):
    m = MATCHERS[which]
    gt, boxes = (t.to(DEV) for t in _scene(family, N, M))
    exp = m(pairwise_iou_rotated(gt, boxes))
    got = m.match_boxes_rotated(gt, boxes)
    assert got[0].dtype == torch.int64 and got[1].dtype == torch.int8 and got[0].shape == got[1].shape == (N,)
    assert torch.equal(got[0], exp[0]) and torch.equal(got[1], exp[1])
    if family == "pile" and M:
        assert exp[1].ne(0).any()  # (the pile does overlap)


@pytest.mark.parametrize("which", list(MATCHERS))
def test_batch_rows_equal_the_single_image_calls(which):
    m = MATCHERS[which]
    N = 2 * MATCH_ROTATED_STRIP + 7
    boxes = _scene("sparse", N, 5)[1].to(DEV)
    gts = [_scene("sparse", N, M, seed=7)[0].to(DEV) for M in (5, 0, 17)]
    matches, labels = m.match_boxes_rotated_batch(gts, boxes)
    assert matches.shape == labels.shape == (3, N)
    for i, g in enumerate(gts):
        one = m.match_boxes_rotated(g, boxes)
        assert torch.equal(matches[i], one[0]) and torch.equal(labels[i], one[1])
    assert m.match_boxes_rotated_batch([], boxes)[0].shape == (0, N)
    assert m.match_boxes_rotated_batch(gts, boxes[:0])[1].shape == (3, 0)


def test_known_answers():
    """reference tests/structures/test_rotated_boxes.py: IoU 0.5 (half of a unit square) and 36 / 84 (two 10 x 6 boxes
    at right angles on one centre), by hand on either side of a threshold."""
    gt = torch.tensor([[0.5, 0.5, 1.0, 1.0, 0.0], [5.0, 5.0, 10.0, 6.0, 55.0]], device=DEV)
    boxes = torch.tensor([[0.25, 0.5, 0.5, 1.0, 0.0], [5.0, 5.0, 10.0, 6.0, -35.0]], device=DEV)
    matches, labels = Matcher([0.45], [0, 1]).match_boxes_rotated(gt, boxes)
    assert matches.tolist() == [0, 1] and labels.tolist() == [1, 0]
    matches, labels = Matcher([0.55], [0, 1], allow_low_quality_matches=True).match_boxes_rotated(gt, boxes)
    assert matches.tolist() == [0, 1] and labels.tolist() == [1, 1]  # each is its ground truth's best
    assert Matcher([0.55], [0, 1]).match_boxes_rotated(gt, boxes)[1].tolist() == [0, 0]
