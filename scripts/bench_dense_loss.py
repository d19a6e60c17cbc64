"""Device time of the fused dense-anchor losses (csrc/dense_loss.hip) against the same loss composed from torch ops the
way the reference composes it (cat of the levels, boolean mask index, one-hot, the focal formula, smooth-L1 on the
foreground rows, autograd), forward + backward, alternating in one process.  RetinaNet at 2 x 800 x 1344: A_l = 151200,
37800, 9450, 2457, 693, K = 80, bf16, about 100 foreground rows per image from a seeded synthetic ground truth.
Also prints the compulsory bytes (logits read twice and written once, plus labels, deltas and boxes) and the share of
HBM peak (8.0 TB/s) the fused forward + backward reach on them.  One JSON line; `--out FILE` also writes it there."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from detectron2_amd.modeling import dense_anchor_losses  # noqa: E402

HBM_PEAK = 8.0e12
LEVELS = [151200, 37800, 9450, 2457, 693]
ALPHA, GAMMA = 0.25, 2.0


def torch_losses(anchors, logits, deltas, labels, boxes, K):
    """retinanet.py:176-205 + box_regression.py:333-345 with plain torch ops (no `.item()`; the mask index still syncs)."""
    valid = labels >= 0
    pos = valid & (labels != K)
    t = F.one_hot(labels[valid], num_classes=K + 1)[:, :-1].to(logits[0].dtype)
    x = torch.cat(logits, dim=1)[valid]
    p = torch.sigmoid(x)
    ce = F.binary_cross_entropy_with_logits(x, t, reduction="none")
    p_t = p * t + (1 - p) * (1 - t)
    cls = (ce * (1 - p_t) ** GAMMA * (ALPHA * t + (1 - ALPHA) * (1 - t))).sum()
    an = torch.cat(anchors)
    w, h = an[:, 2] - an[:, 0], an[:, 3] - an[:, 1]
    cx, cy = an[:, 0] + 0.5 * w, an[:, 1] + 0.5 * h
    tw, th = boxes[..., 2] - boxes[..., 0], boxes[..., 3] - boxes[..., 1]
    tcx, tcy = boxes[..., 0] + 0.5 * tw, boxes[..., 1] + 0.5 * th
    tgt = torch.stack([(tcx - cx) / w, (tcy - cy) / h, torch.log(tw / w), torch.log(th / h)], dim=-1)
    box = (torch.cat(deltas, dim=1)[pos] - tgt[pos]).abs().sum()
    return cls, box


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=2)
    ap.add_argument("--classes", type=int, default=80)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16", "fp32"])
    ap.add_argument("--window", type=float, default=0.3, help="seconds of device time per timing window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dtype = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[a.dtype]
    dev, N, K, R = "cuda", a.images, a.classes, sum(LEVELS)
    g = torch.Generator().manual_seed(0)
    xy = torch.rand(R, 2, generator=g) * torch.tensor([1344.0, 800.0])
    wh = 32 + 480 * torch.rand(R, 2, generator=g)
    anchors = [t.to(dev) for t in torch.cat([xy - 0.5 * wh, xy + 0.5 * wh], dim=1).split(LEVELS)]
    u = torch.rand(N, R, generator=g)
    labels = torch.where(u < 100.0 / R, torch.randint(0, K, (N, R), generator=g), K)
    labels[(u > 0.5) & (u < 0.5 + 500.0 / R)] = -1  # the band between the matcher's thresholds
    an = torch.cat([xy - 0.5 * wh, xy + 0.5 * wh], dim=1)
    boxes = (an[None] + 0.2 * (torch.rand(N, R, 4, generator=g) - 0.5) * torch.cat([wh, wh], dim=1)[None]).to(dev)
    labels = labels.to(dev)
    logits = [(torch.randn(N, A, K, generator=g) - 4).to(dev, dtype).requires_grad_() for A in LEVELS]
    deltas = [(0.2 * torch.randn(N, A, 4, generator=g)).to(dev, dtype).requires_grad_() for A in LEVELS]

    def fused():
        cls, box, _ = dense_anchor_losses(anchors, logits, deltas, labels, boxes, label_mode="class", alpha=ALPHA,
                                          gamma=GAMMA)
        (cls + box).backward()

    def composed():
        cls, box = torch_losses(anchors, logits, deltas, labels, boxes, K)
        (cls + box).backward()

    def window(fn, reps):
        for t in logits + deltas:
            t.grad = None
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
            for t in logits + deltas:
                t.grad = None
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    reps = {}
    for name, fn in (("fused", fused), ("composed", composed)):  # warm-up, and repetitions that fill the window
        window(fn, 3)
        reps[name] = max(5, int(a.window * 1e3 / window(fn, 5)) + 1)
    times = {"fused": [], "composed": []}
    for _ in range(a.rounds):  # alternating
        times["fused"].append(window(fused, reps["fused"]))
        times["composed"].append(window(composed, reps["composed"]))
    es = logits[0].element_size()
    nbytes = 3 * N * R * K * es + 2 * N * R * 4 * es + N * R * (8 + 16) + R * 16
    f_ms, c_ms = statistics.median(times["fused"]), statistics.median(times["composed"])
    res = {"bench": "dense_loss", "device": torch.cuda.get_device_name(0), "images": N, "levels": LEVELS, "classes": K,
           "dtype": a.dtype, "foreground_rows": int(((labels >= 0) & (labels != K)).sum()),
           "fused_fwd_bwd_ms": round(f_ms, 4), "composed_fwd_bwd_ms": round(c_ms, 4), "speedup": round(c_ms / f_ms, 2),
           "fused_windows_ms": [round(t, 4) for t in times["fused"]],
           "composed_windows_ms": [round(t, 4) for t in times["composed"]], "reps_per_window": reps,
           "compulsory_bytes": nbytes, "fused_share_of_hbm_peak": round(nbytes / (f_ms * 1e-3) / HBM_PEAK, 4)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
