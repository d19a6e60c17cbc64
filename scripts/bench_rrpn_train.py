"""Device time of the two fused pieces of rotated-proposal training against what they replace, alternating in one process.

* matcher: `Matcher.match_boxes_rotated_batch` (csrc/matcher_rot.hip) against the composition of rrpn.py:165-197, per
  image `Matcher(pairwise_iou_rotated(gt, anchors))`, at the `rrpn_micro` shape: 2 images x 16 ground-truth boxes x
  268,569 anchors, the inputs of `bench_extra.rotated_inputs` (the standard RPN anchors and `bench.make_boxes` ground
  truth as centre / size rows with an angle ~ U(-180, 180)).  The two results are compared with torch.equal first.
* losses: `rrpn_losses` forward + backward (csrc/rrpn_loss.hip) against the same loss composed from torch ops the way
  RPN.losses composes it (cat of the levels, get_deltas over all anchors, boolean-mask gathers, smooth-L1, BCE,
  autograd), on the same anchors, labels subsampled to 256 per image, bf16 by default.
One JSON line; `--out FILE` also writes it there."""
import argparse
import json
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench as B  # noqa: E402
from detectron2_amd.layers import pairwise_iou_rotated  # noqa: E402
from detectron2_amd.modeling import Matcher, rrpn_label_anchors, rrpn_losses, subsample_anchor_labels_  # noqa: E402

WEIGHTS = (1.0, 1.0, 1.0, 1.0, 1.0)
BETA, BATCH = 0.0, 256


def rot(xyxy, g):
    cx, cy = (xyxy[:, 0] + xyxy[:, 2]) / 2, (xyxy[:, 1] + xyxy[:, 3]) / 2
    ang = torch.empty(xyxy.shape[0]).uniform_(-180, 180, generator=g)
    return torch.stack([cx, cy, xyxy[:, 2] - xyxy[:, 0], xyxy[:, 3] - xyxy[:, 1], ang], 1)


def torch_losses(anchors, logits, deltas, labels, boxes):
    an = torch.cat(anchors)
    x, d = torch.cat(logits, dim=1), torch.cat(deltas, dim=1)
    valid, pos = labels >= 0, labels == 1
    da = (boxes[..., 4] - an[:, 4] + 180.0) % 360.0 - 180.0
    tgt = torch.stack([WEIGHTS[0] * (boxes[..., 0] - an[:, 0]) / an[:, 2], WEIGHTS[1] * (boxes[..., 1] - an[:, 1]) / an[:, 3],
                       WEIGHTS[2] * torch.log(boxes[..., 2] / an[:, 2]), WEIGHTS[3] * torch.log(boxes[..., 3] / an[:, 3]),
                       da * (WEIGHTS[4] * math.pi / 180.0)], dim=-1)
    loc = (d[pos].float() - tgt[pos]).abs().sum()
    cls = F.binary_cross_entropy_with_logits(x[valid].float(), labels[valid].float(), reduction="sum")
    norm = BATCH * labels.shape[0]
    return cls / norm, loc / norm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=2)
    ap.add_argument("--boxes", type=int, default=16, help="ground-truth boxes per image")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16", "fp32"])
    ap.add_argument("--window", type=float, default=0.3, help="seconds of device time per timing window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dtype = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[a.dtype]
    dev, N = "cuda", a.images
    gens = [B.image_generator(1234 + 53, i) for i in range(N)]
    anchors = [rot(lv, gens[0]).to(dev) for lv in B.level_anchors()]
    levels = [len(x) for x in anchors]
    cat = torch.cat(anchors)
    gts = [rot(B.make_boxes(g, a.boxes, 16, 512), g).to(dev) for g in gens]
    matcher = Matcher([0.3, 0.7], [0, -1, 1], allow_low_quality_matches=True)

    def fused_match():
        return matcher.match_boxes_rotated_batch(gts, cat)

    def composed_match():
        return [matcher(pairwise_iou_rotated(g, cat)) for g in gts]

    got, exp = fused_match(), composed_match()
    same = all(torch.equal(got[0][i], e[0]) and torch.equal(got[1][i], e[1]) for i, e in enumerate(exp))

    labels, boxes = rrpn_label_anchors(anchors, gts, matcher)
    subsample_anchor_labels_(labels, BATCH, 0.5, generator=torch.Generator(device=dev).manual_seed(0))
    g = torch.Generator().manual_seed(0)
    logits = [torch.randn(N, A, generator=g).to(dev, dtype).requires_grad_() for A in levels]
    deltas = [(0.3 * torch.randn(N, A, 5, generator=g)).to(dev, dtype).requires_grad_() for A in levels]
    leaves = logits + deltas

    def fused_loss():
        out = rrpn_losses(anchors, logits, labels, deltas, boxes, batch_size_per_image=BATCH, smooth_l1_beta=BETA,
                          box2box_weights=WEIGHTS)
        (out["loss_rpn_cls"] + out["loss_rpn_loc"]).backward()

    def composed_loss():
        cls, loc = torch_losses(anchors, logits, deltas, labels, boxes)
        (cls + loc).backward()

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

    with torch.no_grad():
        out = rrpn_losses(anchors, logits, labels, deltas, boxes, batch_size_per_image=BATCH, smooth_l1_beta=BETA,
                          box2box_weights=WEIGHTS)
        sums = {"fused": [float(out["loss_rpn_cls"]), float(out["loss_rpn_loc"])],
                "composed": [float(v) for v in torch_losses(anchors, logits, deltas, labels, boxes)]}
    fns = {"fused_match": fused_match, "composed_match": composed_match, "fused_loss": fused_loss,
           "composed_loss": composed_loss}
    reps, times = {}, {k: [] for k in fns}
    for name, fn in fns.items():  # warm-up, and repetitions that fill the window
        window(fn, 3)
        reps[name] = max(5, int(a.window * 1e3 / window(fn, 5)) + 1)
    for _ in range(a.rounds):  # alternating
        for name, fn in fns.items():
            times[name].append(window(fn, reps[name]))
    med = {k: statistics.median(v) for k, v in times.items()}
    res = {"bench": "rrpn_train", "device": torch.cuda.get_device_name(0), "images": N, "levels": levels,
           "gt_boxes_per_image": a.boxes, "dtype": a.dtype, "matcher_equal": same,
           "positive_anchors": int((labels == 1).sum()), "valid_anchors": int((labels >= 0).sum()), "loss_sums": sums,
           "fused_match_ms": round(med["fused_match"], 4), "composed_match_ms": round(med["composed_match"], 4),
           "match_speedup": round(med["composed_match"] / med["fused_match"], 2),
           "fused_loss_fwd_bwd_ms": round(med["fused_loss"], 4), "composed_loss_fwd_bwd_ms": round(med["composed_loss"], 4),
           "loss_speedup": round(med["composed_loss"] / med["fused_loss"], 2),
           "windows_ms": {k: [round(t, 4) for t in v] for k, v in times.items()}, "reps_per_window": reps}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
