"""The fused Panoptic FPN merge (detectron2_amd/csrc/panoptic.hip) through the public interface, against a plain restatement
of the reference's loop (modeling/meta_arch/panoptic_fpn.py:184-269) in torch on the CPU.  Every quantity is an integer or a
comparison: every assertion is exact equality."""
import types

import pytest
import torch

from detectron2_amd.layers import paste_masks_in_image
from detectron2_amd.modeling import combine_semantic_and_instance_outputs, panoptic_combine_device

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _reference(scores, classes, masks, sem, overlap, stuff_thresh, score_thresh, num_classes=256):
    """-> (panoptic_seg, segments_info, table rows of the device form, events met on the way)"""
    seg, info, rows, events, cur = torch.zeros(sem.shape, dtype=torch.int32), [], [], [], 0
    for i in torch.argsort(scores, descending=True, stable=True).tolist():
        score = scores[i].item()
        if score < score_thresh:
            events.append("low")
            break
        mask = masks[i].bool()
        area = int(mask.sum())
        if area == 0:
            events.append("empty")
            continue
        inter = int((mask & (seg > 0)).sum())
        if inter * 1.0 / area > overlap:
            events.append("rejected")
            continue
        events.append("truncated" if inter else "whole")
        cur += 1
        seg[mask & (seg == 0)] = cur
        info.append({"id": cur, "isthing": True, "score": score, "category_id": int(classes[i]), "instance_id": i})
        rows.append([cur, 1, int(classes[i]), i, area - inter])
    for label in range(1, num_classes):
        if not (sem == label).any():
            continue
        mask = (sem == label) & (seg == 0)
        area = int(mask.sum())
        if area < stuff_thresh:
            events.append("dropped")
            continue
        cur += 1
        seg[mask] = cur
        info.append({"id": cur, "isthing": False, "category_id": label, "area": area})
        rows.append([cur, 0, label, -1, area])
    return seg, info, rows, events


def _check(scores, classes, masks, sem, overlap, stuff_thresh, score_thresh, num_classes=256, **source):
    """Both public forms against the loop; `source`: the device form's mask source when it is not the pasted `masks`."""
    want_seg, want_info, want_rows, events = _reference(scores, classes, masks, sem, overlap, stuff_thresh, score_thresh,
                                                        num_classes)
    inst = types.SimpleNamespace(scores=scores.to(DEV), pred_classes=classes.to(DEV), pred_masks=masks.to(DEV))
    if num_classes == 256:
        seg, info = combine_semantic_and_instance_outputs(inst, sem.to(DEV), overlap, stuff_thresh, score_thresh)
        assert seg.dtype == torch.int32 and torch.equal(seg.cpu(), want_seg)
        assert info == want_info
    source = source or {"pred_masks": inst.pred_masks}
    out = panoptic_combine_device(inst.scores, inst.pred_classes, sem.to(DEV), overlap, stuff_thresh, score_thresh,
                                  num_classes=num_classes, **source)
    seg, table, count, stats = out
    assert seg.dtype == torch.int32 and torch.equal(seg.cpu(), want_seg)
    assert table.shape == (len(scores) + num_classes, 5) and count.shape == (1,) and stats.shape == (1,)
    assert count.tolist() == [len(want_rows)]
    assert table.tolist() == want_rows + [[0] * 5] * (table.shape[0] - len(want_rows))
    assert stats.tolist() == [int(((sem < 0) | (sem >= num_classes)).sum())]
    return out, events


def _rect(h, w, y0, y1, x0, x1):
    m = torch.zeros(h, w, dtype=torch.bool)
    m[y0:y1, x0:x1] = True
    return m


def test_constructed_rectangles():
    h, w = 37, 70  # no multiple of the 64 x 16 tile
    masks = torch.stack([_rect(h, w, 2, 20, 2, 30),     # accepted whole
                         _rect(h, w, 4, 18, 10, 34),    # 280 of its 336 pixels are the first's: rejected
                         _rect(h, w, 10, 30, 25, 50),   # 50 of 500: accepted, truncated
                         _rect(h, w, 0, 0, 0, 0),       # empty
                         _rect(h, w, 30, 36, 55, 69)])  # below the score threshold
    scores = torch.tensor([0.9, 0.8, 0.7, 0.6, 0.2])
    sem = torch.zeros(h, w, dtype=torch.int64)
    sem[:, 20:45], sem[:, 45:67], sem[:, 67:] = 1, 2, 3  # the last stripe: 111 pixels < 200
    _, events = _check(scores, torch.tensor([3, 1, 4, 1, 5]), masks, sem, 0.5, 200, 0.5)
    assert events == ["whole", "rejected", "truncated", "empty", "low", "dropped"]


def test_128_disjoint_squares_cross_the_set_words():
    g = torch.Generator().manual_seed(1)
    h, w = 64, 128
    masks = torch.stack([_rect(h, w, 8 * (i // 16) + 2, 8 * (i // 16) + 6, 8 * (i % 16) + 1, 8 * (i % 16) + 5)
                         for i in range(128)])
    scores = 0.3 + torch.randperm(128, generator=g).float() / 256
    (_, table, _, _), events = _check(scores, torch.arange(128) % 80, masks, torch.randint(0, 5, (h, w), generator=g), 0.5,
                                      16, 0.05)
    assert events.count("whole") == 128  # ids 32 / 33, 64 / 65 and 96 / 97 are the ranks either side of a set word
    assert table[:128, 3].cpu().tolist() == torch.argsort(scores, descending=True, stable=True).tolist()


def _noise(g):
    # 48 x 72 = 3,456 pixels of (almost surely) distinct 128-bit sets: more keys than the 2,048 slots (PAN_TABLE) of the
    # greedy kernel's LDS table, so the rest is streamed from global memory in every step
    h, w = 48, 72
    return (torch.rand(128, generator=g), torch.randint(0, 80, (128,), generator=g),
            torch.rand(128, h, w, generator=g) < 0.5, torch.randint(0, 5, (h, w), generator=g))


def test_noise_overflows_the_key_table():
    scores, classes, masks, sem = _noise(torch.Generator().manual_seed(2))
    _, events = _check(scores, classes, masks.to(torch.uint8), sem, 0.5, 64, 0.1)
    assert "rejected" in events and "truncated" in events and "low" in events


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fused_paste_equals_pasted_masks(dtype):
    g = torch.Generator().manual_seed(3)
    h, w, r, m = 45, 83, 6, 28
    probs = torch.rand(r, 1, m, m, generator=g).to(dtype)
    boxes = torch.tensor([[5.2, 3.7, 40.9, 30.1], [30.0, 10.5, 95.5, 52.0],  # the second: partly outside the image
                          [50.3, 20.2, 50.9, 40.0],                          # thinner than a pixel
                          [-6.0, -4.0, 20.0, 12.5], [10.0, 25.0, 70.0, 44.0], [60.5, 1.5, 80.0, 20.0]])
    scores, classes = torch.rand(r, generator=g), torch.randint(0, 80, (r,), generator=g)
    sem = torch.randint(0, 4, (h, w), generator=g)
    pasted = paste_masks_in_image(probs[:, 0].to(DEV), boxes.to(DEV), (h, w), 0.5)  # pinned by tests/test_gpu_masks.py
    assert pasted.dtype == torch.bool and pasted[2].any() and not pasted[1].all()
    fused, _ = _check(scores, classes, pasted.cpu(), sem, 0.5, 100, 0.1, num_classes=54,
                      mask_probs=probs.to(DEV), boxes=boxes.to(DEV))
    from_pasted, _ = _check(scores, classes, pasted.cpu(), sem, 0.5, 100, 0.1, num_classes=54)
    assert all(torch.equal(a, b) for a, b in zip(fused, from_pasted))


def test_edge_inputs():
    g = torch.Generator().manual_seed(4)
    h, w = 20, 33
    sem = torch.randint(0, 4, (h, w), generator=g)
    _check(torch.zeros(0), torch.zeros(0, dtype=torch.int64), torch.zeros(0, h, w, dtype=torch.bool), sem, 0.5, 10, 0.5)
    sem[3:9, 5:17] = 7  # outside [0, 6): no segment, pixels 0 unless a thing owns them, counted
    masks = torch.stack([_rect(h, w, 0, 5, 0, 9), _rect(h, w, 12, 20, 20, 33)])
    (seg, _, _, stats), _ = _check(torch.tensor([0.9, 0.8]), torch.tensor([1, 2]), masks, sem, 0.5, 10, 0.5, num_classes=6)
    assert stats.tolist() == [72] and (seg[5:9, 5:17] == 0).all()
    many = (torch.rand(129, device=DEV), torch.zeros(129, dtype=torch.int64, device=DEV), sem.to(DEV), 0.5, 10, 0.5)
    with pytest.raises(NotImplementedError):
        panoptic_combine_device(*many, pred_masks=torch.zeros(129, h, w, dtype=torch.bool, device=DEV))
    two = (torch.tensor([0.9, 0.8]), torch.tensor([1, 2]), sem, 0.5, 10, 0.5)
    with pytest.raises(NotImplementedError):
        panoptic_combine_device(*two, pred_masks=masks)  # CPU tensors
    two = tuple(t.to(DEV) if isinstance(t, torch.Tensor) else t for t in two)
    with pytest.raises(ValueError):
        panoptic_combine_device(*two)
    with pytest.raises(ValueError):
        panoptic_combine_device(*two, pred_masks=masks.to(DEV), mask_probs=torch.rand(2, 28, 28, device=DEV),
                                boxes=torch.zeros(2, 4, device=DEV))


def test_two_runs_are_bit_identical():
    scores, classes, masks, sem = (t.to(DEV) for t in _noise(torch.Generator().manual_seed(5)))
    a, b = (panoptic_combine_device(scores, classes, sem, 0.5, 64, 0.1, pred_masks=masks, num_classes=5) for _ in range(2))
    assert all(torch.equal(x, y) for x, y in zip(a, b))
