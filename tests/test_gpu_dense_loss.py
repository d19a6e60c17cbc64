"""GPU parity of the fused dense-anchor losses (detectron2_amd/csrc/dense_loss.hip) through the public interface, against
the same losses written with plain torch in float64 on the CPU (cat, mask index, one-hot, the focal formula, get_deltas /
apply_deltas, smooth-L1, GIoU with eps 1e-7, autograd for the gradients).
Bars: the keypoint test's, re-derived on these inputs.  The same formulas in fp32 torch on the CPU differ from float64 by
1.3e-7 relative (sums), 6.7e-7 absolute (classification gradient: autograd through (1 - p_t)^gamma * ce with ce = 60 at
the +-60 logits) and 1.4e-5 * max(1, |ref|) (box gradient: (x - target) / beta with beta = 0.11 and a target whose
centre difference cancels at 600 px).  The last two exceed a quarter of the starting bars (1e-6, 1e-5), so those bars
are 4 x the measured fp32 error:
  sums 1e-5 relative; classification gradients 2.7e-6 absolute; box gradients 5.5e-5 * max(1, |ref|);
  16-bit I/O adds one rounding of the I/O dtype (bf16 2^-8, f16 2^-11 relative, f16 subnormal spacing 2^-24).
A wrong target, alpha branch or mask is an O(0.1 - 1) error.  Counts and zeros are exact."""
import math

import pytest
import torch
import torch.nn.functional as F

from detectron2_amd.modeling import (DENSE_LOSS_TILE, Matcher, dense_anchor_losses, retinanet_label_anchors,
                                     retinanet_losses, rpn_losses)

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = DENSE_LOSS_TILE
LEVELS = [2 * T + 5, T + 5, 70, 9, 1]  # several tiles + a ragged tail, a level under a tile, a one-anchor level
CLAMP = math.log(1000.0 / 16)
WEIGHTS = (1.0, 1.0, 2.0, 2.0)
UP = (0.7, 1.3)  # upstream gradients of the two sums
RND = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}


def _inputs(K, dtype, seed, objectness=False):
    """-> anchors[l], logits[l], deltas[l] (values already rounded to dtype), labels [N,R], boxes [N,R,4]; all CPU."""
    g = torch.Generator().manual_seed(seed)
    N, R = 2, sum(LEVELS)
    xy = 600 * torch.rand(R, 2, generator=g)
    wh = 16 + 240 * torch.rand(R, 2, generator=g)
    anchors = torch.cat([xy, xy + wh], dim=1)
    u = torch.rand(N, R, generator=g)
    fg = torch.randint(0, K, (N, R), generator=g)
    labels = torch.where(u < 0.05, -1, torch.where(u > 0.98, fg, K))
    labels[1, T:2 * T] = -1   # one tile wholly ignored
    labels[:, R - 1] = K - 1  # the one-anchor level is foreground
    if objectness:
        labels = torch.where(labels < 0, -1, torch.where(labels < K, 1, 0))
    jit = 1 + 0.3 * (2 * torch.rand(N, R, 4, generator=g) - 1)  # the anchor moved / resized by at most 30 %
    ctr = (xy + 0.5 * wh) + (jit[..., :2] - 1) * wh
    boxes = torch.cat([ctr - 0.5 * wh * jit[..., 2:], ctr + 0.5 * wh * jit[..., 2:]], dim=-1)
    logits, deltas = [], []
    for A in LEVELS:
        x = 3 * torch.randn(N, A, K, generator=g)
        x.view(-1)[torch.randint(0, x.numel(), (6,), generator=g)] = torch.tensor([60.0, -60.0] * 3)
        logits.append(x)
        deltas.append(0.2 * torch.randn(N, A, 4, generator=g))
    deltas[-1][0, 0, 2] = 2 * CLAMP * WEIGHTS[2]  # a foreground row whose dw is clamped
    if dtype == torch.float16:  # saturation where log(p), log(1 - p) taken directly would be -inf
        logits[0][0, 1, 0], logits[0][0, 2, 0] = 6e4, -6e4
        labels[0, 1], labels[0, 2] = (0, 1) if objectness else (K, 0)
    rnd = lambda ts: [t.to(dtype).float() for t in ts]
    return list(anchors.split(LEVELS)), rnd(logits), rnd(deltas), labels, boxes


def _ref(anchors, logits, deltas, labels, boxes, objectness, alpha, gamma, box, beta, dt=torch.float64):
    """-> (loss_cls_sum, loss_box_sum, leaves) in `dt`, composed the way the reference composes them."""
    lg = [x.to(dt).requires_grad_() for x in logits]
    dl = [d.to(dt).requires_grad_() for d in deltas]
    an, gt = torch.cat(anchors).to(dt), boxes.to(dt)
    K = lg[0].shape[-1]
    valid = labels >= 0
    pos = (labels == 1) if objectness else valid & (labels != K)
    x = torch.cat(lg, dim=1)[valid]
    if objectness:
        t = labels[valid].to(dt)[:, None]
    else:
        t = F.one_hot(labels[valid], K + 1)[:, :-1].to(dt)
    ce = x.clamp(min=0) - x * t + torch.log1p(torch.exp(-x.abs()))
    p = torch.sigmoid(x)
    p_t = p * t + (1 - p) * (1 - t)
    loss = ce * (1 - p_t) ** gamma if gamma != 0 else ce
    if alpha >= 0:
        loss = loss * (alpha * t + (1 - alpha) * (1 - t))
    w, h = an[:, 2] - an[:, 0], an[:, 3] - an[:, 1]
    cx, cy = an[:, 0] + 0.5 * w, an[:, 1] + 0.5 * h
    wx, wy, ww, wh = WEIGHTS
    d = torch.cat(dl, dim=1)
    if box == "smooth_l1":
        tw, th = gt[..., 2] - gt[..., 0], gt[..., 3] - gt[..., 1]
        tcx, tcy = gt[..., 0] + 0.5 * tw, gt[..., 1] + 0.5 * th
        tgt = torch.stack([wx * (tcx - cx) / w, wy * (tcy - cy) / h, ww * torch.log(tw / w), wh * torch.log(th / h)], -1)
        n = (d[pos] - tgt[pos]).abs()
        lbox = n if beta < 1e-5 else torch.where(n < beta, 0.5 * n ** 2 / beta, n - 0.5 * beta)
    else:
        pcx, pcy = d[..., 0] / wx * w + cx, d[..., 1] / wy * h + cy
        pw, ph = torch.exp((d[..., 2] / ww).clamp(max=CLAMP)) * w, torch.exp((d[..., 3] / wh).clamp(max=CLAMP)) * h
        x1, y1, x2, y2 = [v[pos] for v in (pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph)]
        X1, Y1, X2, Y2 = gt[pos].unbind(-1)
        iw, ih = torch.min(x2, X2) - torch.max(x1, X1), torch.min(y2, Y2) - torch.max(y1, Y1)
        inter = torch.where((iw > 0) & (ih > 0), iw * ih, torch.zeros_like(iw))
        union = (x2 - x1) * (y2 - y1) + (X2 - X1) * (Y2 - Y1) - inter
        area_c = (torch.max(x2, X2) - torch.min(x1, X1)) * (torch.max(y2, Y2) - torch.min(y1, Y1))
        lbox = 1 - inter / (union + 1e-7) + (area_c - union) / (area_c + 1e-7)
    return loss.sum(), lbox.sum(), lg, dl


def _run(anchors, logits, deltas, labels, boxes, dtype, fn):
    lg = [x.to(DEV, dtype).requires_grad_() for x in logits]
    dl = [d.to(DEV, dtype).requires_grad_() for d in deltas]
    cls, box, *rest = fn([a.to(DEV) for a in anchors], lg, dl, labels.to(DEV), boxes.to(DEV))
    (UP[0] * cls + UP[1] * box).backward()
    return cls, box, rest, [x.grad for x in lg], [d.grad for d in dl]


def _check(got, ref, labels, objectness, dtype, levels=LEVELS):
    cls, box, _, g_lg, g_dl = got
    rcls, rbox, lg, dl = ref
    (UP[0] * rcls + UP[1] * rbox).backward()
    for name, a, b in (("cls", cls, rcls), ("box", box, rbox)):
        a, b = a.detach(), b.detach()
        print(f"{name} sum {float(a):.8g} ref {float(b):.8g}")
        assert a.dtype == torch.float32 and abs(float(a) - float(b)) <= 1e-5 * abs(float(b)), name
    K = lg[0].shape[-1]
    valid = labels >= 0
    pos = (labels == 1) if objectness else valid & (labels != K)
    tiny = 2.0 ** -24 if dtype == torch.float16 else 0.0
    for l, (v, ps) in enumerate(zip(valid.split(levels, dim=1), pos.split(levels, dim=1))):
        a, b = g_lg[l].cpu().double(), lg[l].grad
        assert g_lg[l].dtype == dtype and ((a - b).abs() <= 2.7e-6 + RND[dtype] * b.abs() + tiny).all(), (l, float((a - b).abs().max()))
        assert (a[~v] == 0).all(), l
        a, b = g_dl[l].cpu().double(), dl[l].grad
        assert ((a - b).abs() <= 5.5e-5 * b.abs().clamp(min=1) + RND[dtype] * b.abs() + tiny).all(), (l, float((a - b).abs().max()))
        assert (a[~ps] == 0).all(), l


CASES = [(80, torch.bfloat16, 0.25, 2.0, "smooth_l1", 0.0), (80, torch.bfloat16, 0.25, 2.0, "giou", 0.0),
         (80, torch.float32, 0.25, 2.0, "giou", 0.0), (3, torch.float32, -1.0, 0.0, "smooth_l1", 0.11),
         (3, torch.float16, 0.25, 1.5, "giou", 0.0), (1, torch.float32, 0.25, 1.5, "smooth_l1", 0.0),
         (3, torch.bfloat16, 0.25, 1.5, "smooth_l1", 0.11)]


@pytest.mark.parametrize("K,dtype,alpha,gamma,box,beta", CASES)
def test_class_mode_against_float64(K, dtype, alpha, gamma, box, beta):
    inp = _inputs(K, dtype, seed=K)
    kw = dict(label_mode="class", alpha=alpha, gamma=gamma, box_reg_loss_type=box, smooth_l1_beta=beta, weights=WEIGHTS)
    got = _run(*inp, dtype, lambda a, x, d, lab, gt: dense_anchor_losses(a, x, d, lab, gt, **kw))
    labels = inp[3]
    stats = got[2][0].cpu()
    assert stats.dtype == torch.int64 and stats.tolist() == [int(((labels >= 0) & (labels != K)).sum()), int((labels >= 0).sum())]
    _check(got, _ref(*inp, False, alpha, gamma, box, beta), labels, False, dtype)
    if box == "giou":  # the row whose dw is clamped: no dw gradient, but a dh gradient
        assert float(got[4][-1][0, 0, 2]) == 0.0 and float(got[4][-1][0, 0, 3]) != 0.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_rpn_losses_against_float64_bce(dtype):
    """Objectness labels: 1 is foreground (not "background of a one-class detector"), logits come as [N, A_l]."""
    anchors, logits, deltas, labels, boxes = _inputs(1, dtype, seed=11, objectness=True)

    def fn(a, x, d, lab, gt):
        out = rpn_losses(a, [v.squeeze(-1) for v in x], list(lab), d, list(gt), batch_size_per_image=256,
                         box_reg_loss_type="smooth_l1", smooth_l1_beta=0.11, box2box_weights=WEIGHTS,
                         loss_weight={"loss_rpn_cls": 1.0, "loss_rpn_loc": 2.0})
        return out["loss_rpn_cls"] * 512, out["loss_rpn_loc"] * 256
    got = _run(anchors, logits, deltas, labels, boxes, dtype, fn)
    ref = _ref(anchors, logits, deltas, labels, boxes, True, -1.0, 0.0, "smooth_l1", 0.11)
    v = labels >= 0
    bce = F.binary_cross_entropy_with_logits(torch.cat(logits, 1).double().squeeze(-1)[v], labels[v].double(), reduction="sum")
    assert abs(float(bce) - float(ref[0].detach())) <= 1e-12 * float(bce)
    _check(got, ref, labels, True, dtype)


def test_edge_cases():
    anchors, logits, deltas, labels, boxes = _inputs(3, torch.float32, seed=5)
    kw = dict(label_mode="class", alpha=0.25, gamma=2.0)
    for lab, cls_zero in ((torch.where(labels >= 0, 3, -1), False), (torch.full_like(labels, -1), True)):
        cls, box, (stats,), g_lg, g_dl = _run(anchors, logits, deltas, lab, boxes, torch.float32,
                                              lambda a, x, d, l_, gt: dense_anchor_losses(a, x, d, l_, gt, **kw))
        cls, box = cls.detach(), box.detach()
        assert float(box) == 0.0 and int(stats[0]) == 0 and all(not g.any() for g in g_dl)
        assert (float(cls) == 0.0 and all(not g.any() for g in g_lg) and int(stats[1]) == 0) if cls_zero else float(cls) > 0
    dev = lambda ts: [t.to(DEV) for t in ts]
    for a, x, d, lab, gt in (([], [], [], labels[:, :0], boxes[:, :0]),
                             (anchors, [v[:0] for v in logits], [v[:0] for v in deltas], labels[:0], boxes[:0])):
        cls, box, stats = dense_anchor_losses(dev(a), dev(x), dev(d), lab.to(DEV), gt.to(DEV), **kw)
        assert float(cls) == 0.0 and float(box) == 0.0 and stats.tolist() == [0, 0]
    with pytest.raises(NotImplementedError, match="diou"):
        dense_anchor_losses(anchors, logits, deltas, labels, boxes, box_reg_loss_type="diou", **kw)  # before any launch
    with pytest.raises(NotImplementedError):
        dense_anchor_losses(anchors, logits, deltas, labels, boxes, **kw)  # CPU tensors


def test_two_runs_are_bit_identical():
    inp = _inputs(80, torch.bfloat16, seed=80)
    kw = dict(label_mode="class", alpha=0.25, gamma=2.0, box_reg_loss_type="giou", weights=WEIGHTS)
    a, b = (_run(*inp, torch.bfloat16, lambda a, x, d, lab, gt: dense_anchor_losses(a, x, d, lab, gt, **kw)) for _ in range(2))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert all(torch.equal(p, q) for p, q in zip(a[3] + a[4], b[3] + b[4]))


def test_retinanet_label_anchors_and_losses_without_a_host_read():
    """label_anchors + losses of 2 images, one without ground truth, against the float64 composition; the normaliser is a
    device tensor; the whole forward is captured into a graph (a host read would fail the capture) and replayed."""
    K, sizes = 5, [300, 75, 12]
    g = torch.Generator().manual_seed(3)
    xy = 200 * torch.rand(sum(sizes), 2, generator=g)
    anchors = list(torch.cat([xy, xy + 24 + 72 * torch.rand(sum(sizes), 2, generator=g)], 1).split(sizes))
    an = torch.cat(anchors)
    gt0 = an[[5, 140, 310, 380]] * torch.tensor([1.02, 0.97, 1.05, 0.95])
    cls0 = torch.tensor([4, 0, 2, 2])
    logits = [3 * torch.randn(2, A, K, generator=g) for A in sizes]
    deltas = [0.2 * torch.randn(2, A, 4, generator=g) for A in sizes]
    # float64 composition of retinanet.py:212-255 with Matcher([0.4, 0.5], [0, -1, 1], allow_low_quality_matches=True)
    a64, g64 = an.double(), gt0.double()
    wh = (torch.min(g64[:, None, 2:], a64[None, :, 2:]) - torch.max(g64[:, None, :2], a64[None, :, :2])).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    area = lambda b: (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    iou = inter / (area(g64)[:, None] + area(a64)[None, :] - inter)
    best, idx = iou.max(dim=0)
    q = torch.where(best >= 0.5, 1, torch.where(best >= 0.4, -1, 0))
    q[(iou == iou.max(dim=1, keepdim=True).values).any(dim=0)] = 1
    lab0 = torch.where(q == 0, K, torch.where(q == -1, -1, cls0[idx]))
    labels = torch.stack([lab0, torch.full_like(lab0, K)])
    boxes = torch.stack([gt0[idx], torch.zeros_like(an)])
    assert int((lab0 >= 0).sum() - (lab0 == K).sum()) >= 4 and int((lab0 == -1).sum()) > 0

    dev = lambda ts: [t.to(DEV) for t in ts]
    matcher = Matcher([0.4, 0.5], [0, -1, 1], allow_low_quality_matches=True)
    norm = torch.tensor([37.0], device=DEV)
    lg, dl = [x.requires_grad_() for x in dev(logits)], [d.requires_grad_() for d in dev(deltas)]
    args = (dev(anchors), dev([gt0, gt0[:0]]), dev([cls0, cls0[:0]]))

    def forward():
        lab, gtb = retinanet_label_anchors(args[0], args[1], args[2], matcher, K)
        return lab, gtb, retinanet_losses(args[0], lg, lab, dl, gtb, num_classes=K, normalizer=norm,
                                          box_reg_loss_type="smooth_l1", smooth_l1_beta=0.11, box2box_weights=WEIGHTS)
    lab, gtb, out = forward()
    assert torch.equal(lab.cpu(), labels) and torch.equal(gtb.cpu(), boxes)
    (UP[0] * out["loss_cls"] * 37 + UP[1] * out["loss_box_reg"] * 37).backward()
    ref = _ref(anchors, logits, deltas, labels, boxes, False, 0.25, 2.0, "smooth_l1", 0.11)
    _check((out["loss_cls"] * 37, out["loss_box_reg"] * 37, None, [x.grad for x in lg], [d.grad for d in dl]), ref, labels,
           False, torch.float32, sizes)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        _, _, captured = forward()
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(captured[k], out[k].detach()) for k in out)
