"""Device time of the fused FCOS training losses (csrc/fcos.hip: matching + focal + GIoU + centerness, forward + backward)
against the same loss composed from torch ops the way the reference composes it (per image the (M, R, 4) distance tensor and
the (M, R) tests of `_match_anchors`, then cat of the levels, one-hot, the focal formula, boolean-mask gathers, GIoU and
the centerness BCE, autograd), alternating in one process.  FCOS R50-FPN at 2 x 800 x 1344: A_l = 16800, 4200, 1050, 273,
77 (22,400 points per image), K = 80, bf16, a seeded synthetic ground truth of `--boxes` boxes per image.
Also prints the compulsory bytes (logits read twice and written once, deltas / centerness / anchors / ground truth, the
int32 `matched` written and read) and the share of HBM peak (8.0 TB/s) the fused forward + backward reach on them.
One JSON line; `--out FILE` also writes it there."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from detectron2_amd.modeling import fcos_losses_from_gt  # noqa: E402

HBM_PEAK = 8.0e12
H, W, STRIDES = 800, 1344, (8, 16, 32, 64, 128)
ALPHA, GAMMA, RADIUS = 0.25, 2.0, 1.5


def torch_losses(anchors, logits, deltas, ctrness, gt_boxes, gt_classes, K):
    """fcos.py:113-251 with plain torch ops (no `.item()`; the mask indices still synchronise)."""
    an = torch.cat(anchors)
    ctr, size = (an[:, :2] + an[:, 2:]) / 2, an[:, 2] - an[:, 0]
    lower, upper = size * 4, size * 8
    lower[:len(anchors[0])] = 0
    upper[-len(anchors[-1]):] = float("inf")
    labels, boxes = [], []
    for gt, cl in zip(gt_boxes, gt_classes):
        q = (ctr[None] - ((gt[:, :2] + gt[:, 2:]) / 2)[:, None]).abs_().max(dim=2).values < RADIUS * size[None]
        x, y = ctr[:, 0, None], ctr[:, 1, None]
        dist = torch.stack([x - gt[None, :, 0], y - gt[None, :, 1], gt[None, :, 2] - x, gt[None, :, 3] - y], 2).permute(1, 0, 2)
        q &= dist.min(dim=2).values > 0
        far = dist.max(dim=2).values
        q &= (far > lower[None]) & (far < upper[None])
        quality, idx = (q.to(torch.float32) * (1e8 - (gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1]))[:, None]).max(dim=0)
        idx[quality < 1e-5] = -1
        lab = cl[idx.clip(min=0)]
        lab[idx < 0] = K
        labels.append(lab), boxes.append(gt[idx.clip(min=0)])
    labels, gt = torch.stack(labels), torch.stack(boxes)
    pos = labels != K
    x, t = torch.cat(logits, dim=1), F.one_hot(labels, num_classes=K + 1)[:, :, :-1].to(logits[0].dtype)
    p = torch.sigmoid(x)
    ce = F.binary_cross_entropy_with_logits(x, t, reduction="none")
    cls = (ce * (1 - (p * t + (1 - p) * (1 - t))) ** GAMMA * (ALPHA * t + (1 - ALPHA) * (1 - t))).sum()
    cx, cy = 0.5 * (an[:, 0] + an[:, 2]), 0.5 * (an[:, 1] + an[:, 3])
    s = torch.stack([size, an[:, 3] - an[:, 1]] * 2, dim=1)
    d = F.relu(torch.cat(deltas, dim=1)) * s
    x1, y1, x2, y2 = (v[pos] for v in (cx - d[..., 0], cy - d[..., 1], cx + d[..., 2], cy + d[..., 3]))
    X1, Y1, X2, Y2 = gt[pos].unbind(-1)
    iw, ih = torch.min(x2, X2) - torch.max(x1, X1), torch.min(y2, Y2) - torch.max(y1, Y1)
    inter = torch.where((iw > 0) & (ih > 0), iw * ih, torch.zeros_like(iw))
    union = (x2 - x1) * (y2 - y1) + (X2 - X1) * (Y2 - Y1) - inter
    hull = (torch.max(x2, X2) - torch.min(x1, X1)) * (torch.max(y2, Y2) - torch.min(y1, Y1))
    loc = (1 - inter / (union + 1e-7) + (hull - union) / (hull + 1e-7)).sum()
    tg = torch.stack([cx - gt[..., 0], cy - gt[..., 1], gt[..., 2] - cx, gt[..., 3] - cy], dim=-1) / s
    lr, tb = tg[..., [0, 2]], tg[..., [1, 3]]
    tc = torch.sqrt(lr.min(-1)[0] / lr.max(-1)[0] * (tb.min(-1)[0] / tb.max(-1)[0]))
    c = torch.cat(ctrness, dim=1).squeeze(2)
    return cls, loc, F.binary_cross_entropy_with_logits(c[pos], tc[pos].to(c.dtype), reduction="sum")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=2)
    ap.add_argument("--classes", type=int, default=80)
    ap.add_argument("--boxes", type=int, default=8, help="ground-truth boxes per image")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16", "fp32"])
    ap.add_argument("--window", type=float, default=0.3, help="seconds of device time per timing window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dtype = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[a.dtype]
    dev, N, K = "cuda", a.images, a.classes
    g = torch.Generator().manual_seed(0)
    anchors = []
    for s in STRIDES:
        ys, xs = torch.meshgrid(torch.arange(0, H, s), torch.arange(0, W, s), indexing="ij")
        c = torch.stack([xs.reshape(-1), ys.reshape(-1)], dim=1).float()
        anchors.append(torch.cat([c - s / 2, c + s / 2], dim=1).to(dev))
    levels = [len(x) for x in anchors]
    R = sum(levels)
    gt_boxes, gt_classes = [], []
    for _ in range(N):
        stride = torch.tensor(STRIDES)[torch.randint(0, 5, (a.boxes,), generator=g)].float()
        ctr = torch.rand(a.boxes, 2, generator=g) * torch.tensor([W, H])
        ext = stride[:, None] * (2.5 + 4.5 * torch.rand(a.boxes, 4, generator=g))
        gt_boxes.append(torch.cat([ctr - ext[:, :2], ctr + ext[:, 2:]], dim=1).to(dev))
        gt_classes.append(torch.randint(0, K, (a.boxes,), generator=g).to(dev))
    logits = [(torch.randn(N, A, K, generator=g) - 4).to(dev, dtype).requires_grad_() for A in levels]
    deltas = [(0.5 * torch.randn(N, A, 4, generator=g) + 0.5).to(dev, dtype).requires_grad_() for A in levels]
    ctrness = [torch.randn(N, A, 1, generator=g).to(dev, dtype).requires_grad_() for A in levels]
    leaves = logits + deltas + ctrness
    positives = []

    def fused():
        cls, loc, ctr, stats = fcos_losses_from_gt(anchors, logits, deltas, ctrness, gt_boxes, gt_classes, num_classes=K,
                                                   center_sampling_radius=RADIUS, alpha=ALPHA, gamma=GAMMA)
        (cls + loc + ctr).backward()
        positives[:] = [stats]

    def composed():
        cls, loc, ctr = torch_losses(anchors, logits, deltas, ctrness, gt_boxes, gt_classes, K)
        (cls + loc + ctr).backward()

    def window(fn, reps):
        for t in leaves:
            t.grad = None
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
            for t in leaves:
                t.grad = None
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    with torch.no_grad():  # the two compute the same thing at this size (the composition accumulates in the I/O dtype)
        sums = {"fused": [float(v) for v in fcos_losses_from_gt(anchors, logits, deltas, ctrness, gt_boxes, gt_classes,
                                                                num_classes=K, alpha=ALPHA, gamma=GAMMA)[:3]],
                "composed": [float(v) for v in torch_losses(anchors, logits, deltas, ctrness, gt_boxes, gt_classes, K)]}
    reps = {}
    for name, fn in (("fused", fused), ("composed", composed)):  # warm-up, and repetitions that fill the window
        window(fn, 3)
        reps[name] = max(5, int(a.window * 1e3 / window(fn, 5)) + 1)
    times = {"fused": [], "composed": []}
    for _ in range(a.rounds):  # alternating
        times["fused"].append(window(fused, reps["fused"]))
        times["composed"].append(window(composed, reps["composed"]))
    es = logits[0].element_size()
    # logits read twice and written once; delta + centerness gradients written, centerness read by the forward; `matched`
    # written and read; the anchors read by every image in both passes; the packed ground truth
    nbytes = 3 * N * R * K * es + 6 * N * R * es + 2 * N * R * 4 + 2 * N * R * 16 + 2 * N * a.boxes * 24
    f_ms, c_ms = statistics.median(times["fused"]), statistics.median(times["composed"])
    res = {"bench": "fcos_loss", "device": torch.cuda.get_device_name(0), "images": N, "levels": levels, "classes": K,
           "dtype": a.dtype, "gt_boxes_per_image": a.boxes, "positive_points": int(positives[0][0]), "loss_sums": sums,
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
