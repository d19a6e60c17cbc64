"""The fused Panoptic FPN merge (csrc/panoptic.hip) against the composition of torch ops the reference runs -- the paste of
the soft masks (layers/mask_ops.py: a sampling grid, F.grid_sample, the threshold) and then the host loop of
combine_semantic_and_instance_outputs (panoptic_fpn.py:184-269), restated here -- same GPU, same process.  800 x 1333,
100 detections from seeded boxes with a trained-model-like score spread, 28 x 28 soft masks, 54 classes; two sets of
boxes: `spread`, and `overlap`, in which about a third of the detections are near-duplicates the merge rejects.  Per case:
median device time of each of the three kernels (and of the paste kernel the pasted form needs first), median
end-to-end host time per image (a host clock around work that ends in a synchronise), host synchronisations per image.
Results are compared at the timed size.  One JSON line per measurement; `--out FILE` also writes them."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time
import types

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from detectron2_amd import _C  # noqa: E402
from detectron2_amd.layers import paste_masks_in_image  # noqa: E402
from detectron2_amd.modeling import combine_semantic_and_instance_outputs, panoptic_combine_device  # noqa: E402

KERNELS = ("paste_masks", "panoptic_coverage", "panoptic_greedy", "panoptic_write")


def torch_paste(probs, boxes, h, w, threshold=0.5, chunk=25):  # mask_ops.py: the device path samples the whole image
    out = []
    ys, xs = torch.arange(h, device=probs.device) + 0.5, torch.arange(w, device=probs.device) + 0.5
    for p, b in zip(probs.split(chunk), boxes.split(chunk)):
        x0, y0, x1, y1 = b.split(1, dim=1)
        gy, gx = (ys - y0) / (y1 - y0) * 2 - 1, (xs - x0) / (x1 - x0) * 2 - 1
        grid = torch.stack([gx[:, None, :].expand(-1, h, -1), gy[:, :, None].expand(-1, -1, w)], dim=3)
        out.append(F.grid_sample(p[:, None].float(), grid, align_corners=False)[:, 0] >= threshold)
    return torch.cat(out)


def torch_combine(scores, classes, masks, sem, overlap, stuff_thresh, score_thresh, reads):
    """The reference's loop; `reads[0]` counts its host synchronisations."""
    seg, info, cur = torch.zeros_like(sem, dtype=torch.int32), [], 0
    for i in torch.argsort(-scores):
        score = scores[i].item()
        reads[0] += 1
        if score < score_thresh:
            break
        mask = masks[i]
        area = mask.sum().item()
        reads[0] += 1
        if area == 0:
            continue
        inter = ((mask > 0) & (seg > 0)).sum().item()
        reads[0] += 1
        if inter * 1.0 / area > overlap:
            continue
        if inter > 0:
            mask = mask & (seg == 0)
        cur += 1
        seg[mask] = cur
        info.append({"id": cur, "isthing": True, "score": score, "category_id": classes[i].item(), "instance_id": i.item()})
        reads[0] += 2
    labels = torch.unique(sem).cpu().tolist()
    reads[0] += 1
    for label in labels:
        if label == 0:
            continue
        mask = (sem == label) & (seg == 0)
        area = mask.sum().item()
        reads[0] += 1
        if area < stuff_thresh:
            continue
        cur += 1
        seg[mask] = cur
        info.append({"id": cur, "isthing": False, "category_id": label, "area": area})
    return seg, info


def detections(g, r, h, w, duplicates):
    """Seeded boxes, descending-ish scores (a few confident, a long tail), blob-shaped soft masks."""
    n = r - duplicates
    size = torch.exp(torch.empty(n).uniform_(3.4, 5.8, generator=g))
    ar = torch.exp(torch.empty(n).uniform_(-0.7, 0.7, generator=g))
    bw, bh = size * ar.sqrt(), size / ar.sqrt()
    cx, cy = torch.empty(n).uniform_(0, w, generator=g), torch.empty(n).uniform_(0, h, generator=g)
    boxes = torch.stack([cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2], 1)
    if duplicates:  # jittered copies: what NMS leaves of one object at a lower score
        src = boxes[torch.randint(0, n, (duplicates,), generator=g)]
        boxes = torch.cat([boxes, src + torch.empty(duplicates, 4).uniform_(-3, 3, generator=g)])
    scores = torch.rand(r, generator=g) ** 3 * 0.95 + 0.05
    if duplicates:
        scores[n:] *= 0.5
    t = torch.linspace(-1, 1, 28)
    rad = (t[None, :, None] ** 2 + t[None, None, :] ** 2).sqrt() * torch.empty(r, 1, 1).uniform_(0.9, 1.3, generator=g)
    probs = torch.sigmoid((1 - rad) * 6 + 0.3 * torch.randn(r, 28, 28, generator=g))
    return boxes, scores.clamp(max=1.0), torch.randint(0, 80, (r,), generator=g), probs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rep", type=int, default=50)
    ap.add_argument("--size", type=int, nargs=2, default=[800, 1333], metavar=("H", "W"))
    ap.add_argument("--detections", type=int, default=100)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("panoptic_bench: no GPU (there is no CPU path to time)")
    dev = torch.device("cuda", 0)
    (h, w), r, nc = args.size, args.detections, 54
    overlap, stuff_thresh, score_thresh = 0.5, 4096, 0.05  # (every detection enters the loop)
    L = _C.lib()
    res = []

    def emit(**kw):
        res.append(kw)
        print(json.dumps(kw), flush=True)

    def host_ms(fn, rep):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(rep):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts)

    def kernel_us(fn, rep):
        per = {k: [] for k in KERNELS}
        for _ in range(rep):
            L.d2amd_timing_select(",".join(KERNELS).encode())
            fn()
            for k in KERNELS:
                ms, n = ctypes.c_double(), ctypes.c_int()
                L.d2amd_timing_read(k.encode(), ctypes.byref(ms), ctypes.byref(n))
                if n.value:
                    per[k].append(ms.value * 1e3)
        L.d2amd_timing_select(b"")
        return {k: statistics.median(v) for k, v in per.items() if v}

    g = torch.Generator().manual_seed(0)
    coarse = torch.randint(0, nc, (-(-h // 64), -(-w // 64)), generator=g)
    sem = coarse.repeat_interleave(64, 0).repeat_interleave(64, 1)[:h, :w].contiguous().to(dev)
    for name, duplicates in (("spread", 0), ("overlap", r // 3)):
        boxes, scores, classes, probs = (t.to(dev) for t in detections(g, r, h, w, duplicates))
        cfg = (overlap, stuff_thresh, score_thresh)
        pasted = paste_masks_in_image(probs, boxes, (h, w), 0.5)
        inst = types.SimpleNamespace(scores=scores, pred_classes=classes, pred_masks=pasted)
        reads = [0]
        # (the expected result from THIS library's paste, bit-exact to the reference's CPU path; torch's device
        # grid_sample may round a sample at the threshold the other way: counted, not asserted)
        want_seg, want_info = torch_combine(scores, classes, pasted, sem, *cfg, reads)
        syncs = reads[0]
        paste_diff = int((torch_paste(probs, boxes, h, w) != pasted).sum())

        def baseline():
            return torch_combine(scores, classes, torch_paste(probs, boxes, h, w), sem, *cfg, [0])

        def paste_then_dropin():
            inst.pred_masks = paste_masks_in_image(probs, boxes, (h, w), 0.5)
            return combine_semantic_and_instance_outputs(inst, sem, *cfg)

        def paste_then_device():
            return panoptic_combine_device(scores, classes, sem, *cfg, num_classes=nc,
                                           pred_masks=paste_masks_in_image(probs, boxes, (h, w), 0.5))

        def fused_device():
            return panoptic_combine_device(scores, classes, sem, *cfg, mask_probs=probs, boxes=boxes, num_classes=nc)

        seg_d, info_d = paste_then_dropin()
        things = sum(1 for d in want_info if d["isthing"])
        candidates = int((scores >= score_thresh).sum())
        equal = {"dropin_seg": bool(torch.equal(seg_d, want_seg)), "dropin_info": info_d == want_info,
                 "pasted_device_seg": bool(torch.equal(paste_then_device()[0], want_seg)),
                 "fused_device_seg": bool(torch.equal(fused_device()[0], want_seg))}
        common = dict(op="panoptic_combine", boxes=name, shape=[h, w], detections=r, candidates=candidates,
                      things_accepted=things, segments=len(want_info), mask=28, classes=nc)
        emit(**common, case="torch_paste_then_loop", host_ms_per_image=host_ms(baseline, max(3, args.rep // 10)),
             host_syncs_per_image=syncs, torch_paste_pixels_differing_from_paste_kernel=paste_diff)
        for case, fn, n_sync in (("paste_then_dropin", paste_then_dropin, 1), ("paste_then_device", paste_then_device, 0),
                                 ("fused_device", fused_device, 0)):
            k = kernel_us(fn, args.rep)
            emit(**common, case=case, kernel_us=k, device_us_sum=sum(k.values()), host_ms_per_image=host_ms(fn, args.rep),
                 host_syncs_per_image=n_sync, equal_to_torch=equal)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
