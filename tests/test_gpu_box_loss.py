"""GPU parity of the fused box-head loss (detectron2_amd/csrc/box_loss.hip) through `fast_rcnn_losses_with_stats`, against a
float64 CPU reference written with plain torch (F.cross_entropy / F.binary_cross_entropy_with_logits, get_deltas /
apply_deltas, fvcore's smooth-L1 and GIoU formulas, autograd), fed the same rounded inputs.
Bars (those of tests/test_gpu_keypoint_head.py): statistics exact; losses 1e-5 relative; fp32 gradients 1e-6 absolute on
grad * rows (a unit-scale quantity); 16-bit I/O: one rounding of the I/O dtype (bf16 2^-8, f16 2^-11 relative, f16
subnormal spacing 2^-24) on top; zeros of padding rows and of non-target delta columns exact."""
import math

import pytest
import torch
import torch.nn.functional as F

from detectron2_amd.modeling import fast_rcnn_losses_with_stats

pytestmark = pytest.mark.gpu
DEV = "cuda"
WEIGHTS, CLAMP = (10.0, 10.0, 5.0, 5.0), math.log(1000.0 / 16)
UP_CLS, UP_BOX = 1.75, 0.5  # upstream gradients of the two losses (different: a swap would show)


def _reference(scores, deltas, classes, boxes, gt, mode, cw, box, beta):
    """-> (loss_cls, loss_box, stats[5], grad_scores, grad_deltas, rows) in float64; the gradient is that of
    UP_CLS * loss_cls + UP_BOX * loss_box."""
    K = scores.shape[1] - 1
    x, d = scores.double().requires_grad_(True), deltas.double().requires_grad_(True)
    keep, fg = (classes >= 0) & (classes <= K), (classes >= 0) & (classes < K)
    rows = int(keep.sum())
    pred = scores.float().argmax(dim=1)  # (CPU: the first of equal maxima)
    stats = [rows, int(fg.sum()), int((pred == classes)[keep].sum()), int((pred == classes)[fg].sum()),
             int((pred == K)[fg].sum())]
    if rows == 0:
        return 0.0, 0.0, stats, torch.zeros_like(x), torch.zeros_like(d), 1
    xs, cs = x[keep], classes[keep]
    if mode == "softmax":
        cls = F.cross_entropy(xs, cs, reduction="sum") / rows
    else:
        t = F.one_hot(cs, K + 1)[:, :K].double()
        el = F.binary_cross_entropy_with_logits(xs[:, :K], t, reduction="none")
        cls = (el * (cw.double() if cw is not None else 1.0)).sum() / rows
    idx = fg.nonzero()[:, 0]
    dd = d[idx] if d.shape[1] == 4 else d.view(-1, K, 4)[idx, classes[idx]]
    pb, gb = boxes.double()[idx], gt.double()[idx]
    w, h = pb[:, 2] - pb[:, 0], pb[:, 3] - pb[:, 1]
    cx, cy = pb[:, 0] + 0.5 * w, pb[:, 1] + 0.5 * h
    wx, wy, ww, wh = WEIGHTS
    if box == "giou":  # apply_deltas (box_regression.py:88-116), then fvcore giou_loss (eps 1e-7)
        dw, dh = (dd[:, 2] / ww).clamp(max=CLAMP), (dd[:, 3] / wh).clamp(max=CLAMP)
        pcx, pcy, pw, ph = dd[:, 0] / wx * w + cx, dd[:, 1] / wy * h + cy, dw.exp() * w, dh.exp() * h
        x1, y1, x2, y2 = pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph
        iw, ih = torch.min(x2, gb[:, 2]) - torch.max(x1, gb[:, 0]), torch.min(y2, gb[:, 3]) - torch.max(y1, gb[:, 1])
        inter = torch.where((iw > 0) & (ih > 0), iw * ih, torch.zeros_like(iw))
        union = (x2 - x1) * (y2 - y1) + (gb[:, 2] - gb[:, 0]) * (gb[:, 3] - gb[:, 1]) - inter
        hull = ((torch.max(x2, gb[:, 2]) - torch.min(x1, gb[:, 0])) * (torch.max(y2, gb[:, 3]) - torch.min(y1, gb[:, 1])))
        lbox = (1 - inter / (union + 1e-7) + (hull - union) / (hull + 1e-7)).sum() / rows
    else:  # get_deltas (box_regression.py:43-86), then fvcore smooth_l1_loss
        tw, th = gb[:, 2] - gb[:, 0], gb[:, 3] - gb[:, 1]
        tgt = torch.stack([wx * (gb[:, 0] + 0.5 * tw - cx) / w, wy * (gb[:, 1] + 0.5 * th - cy) / h,
                           ww * torch.log(tw / w), wh * torch.log(th / h)], dim=1)
        n = (dd - tgt).abs()
        lbox = (n if beta < 1e-5 else torch.where(n < beta, 0.5 * n * n / beta, n - 0.5 * beta)).sum() / rows
    (UP_CLS * cls + UP_BOX * lbox).backward()
    return float(cls.detach()), float(lbox.detach()), stats, x.grad, (d.grad if d.grad is not None else torch.zeros_like(d)), rows


def _inputs(R, K, dtype, agnostic, seed):
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(R, generator=g)
    classes = torch.where(u < 0.4, torch.randint(0, K, (R,), generator=g), torch.where(u < 0.8, K, -1))
    scores = 3 * torch.randn(R, K + 1, generator=g)
    hit = (torch.rand(R, generator=g) < 0.5) & (classes >= 0)
    scores[hit, classes[hit]] += 6  # (so that argmax == class happens)
    classes[0] = 0  # always one foreground row
    if R >= 8:
        classes[0], classes[R - 1] = -1, -1          # padding first and last
        classes[1], scores[1] = 1 % K, 0.5           # all logits equal: the argmax is column 0
        classes[2], scores[2] = K, 80.0              # +-80
        scores[2, 1::2] = -80.0
        classes[3] = K - 1                           # the last foreground class
        classes[4] = 0
    xy, wh = 400 * torch.rand(R, 2, generator=g), 20 + 200 * torch.rand(R, 2, generator=g)
    boxes = torch.cat([xy, xy + wh], dim=1)
    gxy = xy + 0.15 * wh * torch.randn(R, 2, generator=g)
    gt = torch.cat([gxy, gxy + wh * (0.8 + 0.4 * torch.rand(R, 2, generator=g))], dim=1)
    deltas = 0.5 * torch.randn(R, 4 if agnostic else 4 * K, generator=g)
    if R >= 8:
        deltas[4, 2] = 30.0  # class 0's dw / ww above scale_clamp: clamped under giou, no gradient there
    return scores.to(dtype), deltas.to(dtype), classes, boxes, gt


def _check(got, want, dtype, tag):
    losses, stats, g_sc, g_dl = got
    w_cls, w_box, w_stats, w_gsc, w_gdl, rows = want
    assert stats.dtype == torch.int64 and stats.tolist() == w_stats, (stats.tolist(), w_stats)
    eps = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}[dtype]
    sub = 2.0 ** -24 if dtype == torch.float16 else 0.0
    for name, have, ref in (("loss_cls", losses["loss_cls"], w_cls), ("loss_box_reg", losses["loss_box_reg"], w_box)):
        print(f"{tag} {name} {float(have):.8g} want {ref:.8g} rel {abs(float(have) - ref) / max(abs(ref), 1e-30):.3g}")
    for name, have, ref in (("grad_scores", g_sc, w_gsc), ("grad_deltas", g_dl, w_gdl)):
        err = (have.double().cpu() - ref).abs() * rows
        bound = 1e-6 + eps * ref.abs() * rows + sub * rows
        print(f"{tag} {name}: max err * rows {float(err.max()):.3g}, worst err / bound {float((err / bound).max()):.3g}")
    assert abs(float(losses["loss_cls"]) - w_cls) <= 1e-5 * abs(w_cls)
    assert abs(float(losses["loss_box_reg"]) - w_box) <= 1e-5 * abs(w_box)
    for have, ref in ((g_sc, w_gsc), (g_dl, w_gdl)):
        assert have.dtype == dtype
        err = (have.double().cpu() - ref).abs() * rows
        assert (err <= 1e-6 + eps * ref.abs() * rows + sub * rows).all()
        assert (have.cpu()[ref == 0] == 0).all()  # padding rows, the background column, non-target deltas: exact zeros


def _run(scores, deltas, classes, boxes, gt, mode, cw, box, beta, **form):
    sc, dl = scores.to(DEV).requires_grad_(True), deltas.to(DEV).requires_grad_(True)
    losses, stats = fast_rcnn_losses_with_stats(
        sc, dl, classes.to(DEV), boxes.to(DEV), gt.to(DEV), box_reg_loss_type="giou" if box == "giou" else "smooth_l1",
        smooth_l1_beta=beta, box2box_weights=WEIGHTS, scale_clamp=CLAMP, use_sigmoid_ce=mode != "softmax",
        class_weight=None if cw is None else cw.to(DEV), **form)
    (UP_CLS * losses["loss_cls"] + UP_BOX * losses["loss_box_reg"]).backward()
    return {k: v.detach().cpu() for k, v in losses.items()}, stats.cpu(), sc.grad, dl.grad


MODES, BOXES = ("softmax", "sigmoid", "sigmoid_w"), (("l1", 0.0), ("sl1", 0.5), ("giou", 0.0))
CASES = [(67, 80, (torch.float32, torch.bfloat16)[(i + j) % 2], (i + j) % 2 == 1, m, b)
         for i, m in enumerate(MODES) for j, b in enumerate(BOXES)]
CASES += [(67, 80, torch.float16, False, "softmax", BOXES[2]),
          (1, 1, torch.float32, False, "softmax", BOXES[0]), (1, 1, torch.bfloat16, True, "sigmoid", BOXES[2]),
          # more than one pass of a wave over a row, more than one workgroup record
          (130, 1203, torch.float32, False, "softmax", BOXES[1]), (130, 1203, torch.bfloat16, False, "sigmoid_w", BOXES[2]),
          (130, 1203, torch.bfloat16, True, "softmax", BOXES[0]),
          # 8 rows per workgroup: two rows per wave
          (2100, 5, torch.float32, False, "sigmoid", BOXES[2]), (2100, 5, torch.bfloat16, True, "softmax", BOXES[1])]


@pytest.mark.parametrize("R,K,dtype,agnostic,mode,box", CASES,
                         ids=[f"{c[0]}x{c[1]}-{str(c[2])[6:]}-{'agn' if c[3] else 'cls'}-{c[4]}-{c[5][0]}" for c in CASES])
def test_parity(R, K, dtype, agnostic, mode, box):
    scores, deltas, classes, boxes, gt = _inputs(R, K, dtype, agnostic, seed=R + K)
    cw = (torch.rand(K, generator=torch.Generator().manual_seed(K)) < 0.6).float() if mode == "sigmoid_w" else None
    want = _reference(scores, deltas, classes, boxes, gt, mode, cw, box[0], box[1])
    assert 0 < want[2][1] and (R == 1 or want[2][1] < want[2][0] < R)  # foreground, background and padding rows
    got = _run(scores, deltas, classes, boxes, gt, mode, cw, box[0], box[1])
    _check(got, want, dtype, f"[{R}x{K}]")


@pytest.mark.parametrize("R", [0, 37])
def test_nothing_counts(R):
    scores, deltas, classes, boxes, gt = _inputs(max(R, 1), 7, torch.float32, False, seed=5)
    scores, deltas, classes, boxes, gt = scores[:R], deltas[:R], torch.full((R,), -1), boxes[:R], gt[:R]
    scores[:, 0] = float("nan")  # a padding row's logits are not used
    losses, stats, g_sc, g_dl = _run(scores, deltas, classes, boxes, gt, "softmax", None, "l1", 0.0)
    assert float(losses["loss_cls"]) == 0.0 and float(losses["loss_box_reg"]) == 0.0 and stats.tolist() == [0] * 5
    assert g_sc.shape == scores.shape and g_dl.shape == deltas.shape
    assert (g_sc == 0).all() and (g_dl == 0).all()  # (a NaN compares unequal)


def test_sampler_form_replays_in_a_graph():
    """The sampler's fixed-shape rows (N = 2, S = 32; gt_index into the stacked ground truth) captured forward + backward:
    between replays the classes, the matches and the logits are rewritten in place, so the row and foreground counts
    change; every replay against the float64 reference, and two eager runs bit for bit."""
    N, S, K, sizes = 2, 32, 6, [3, 4]
    offsets = torch.tensor([0, 3])
    variants = []
    for seed, fill in ((1, 20), (2, 29), (3, 9)):  # rows 20 .. 31 / 29 .. / 9 .. of every image are padding
        scores, deltas, classes, boxes, _ = _inputs(N * S, K, torch.bfloat16, False, seed)
        classes.view(N, S)[:, fill:] = -1
        g = torch.Generator().manual_seed(seed)
        index = torch.stack([torch.randint(0, n, (S,), generator=g) for n in sizes])
        variants.append((scores, classes.view(N, S).clone(), index))
    _, _, _, boxes, gt_rows = _inputs(N * S, K, torch.bfloat16, False, 1)
    table = gt_rows[:sum(sizes)].clone()
    wants = [_reference(sc, deltas, cl.view(-1), boxes, table[(offsets[:, None] + ix).view(-1)], "softmax", None, "sl1", 0.5)
             for sc, cl, ix in variants]
    assert len({(w[2][0], w[2][1]) for w in wants}) == 3  # the counts differ between the variants
    sc, cl, ix = (t.to(DEV).clone() for t in variants[0])
    dl, bx, tb, off = deltas.to(DEV), boxes.view(N, S, 4).to(DEV), table.to(DEV), offsets.to(DEV)

    def step():
        a, b = sc.detach().requires_grad_(True), dl.detach().requires_grad_(True)
        losses, stats = fast_rcnn_losses_with_stats(a, b, cl, bx, tb, gt_index=ix, gt_offsets=off, rows_per_image=S,
                                                    smooth_l1_beta=0.5, box2box_weights=WEIGHTS, scale_clamp=CLAMP)
        g_a, g_b = torch.autograd.grad(UP_CLS * losses["loss_cls"] + UP_BOX * losses["loss_box_reg"], [a, b])
        return losses["loss_cls"].detach(), losses["loss_box_reg"].detach(), stats, g_a, g_b

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = [[t.clone() for t in step()] for _ in range(2)]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(*eager))  # deterministic
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    for (v_sc, v_cl, v_ix), want in list(zip(variants, wants))[1:] + [(variants[0], wants[0])]:
        sc.copy_(v_sc); cl.copy_(v_cl); ix.copy_(v_ix)
        graph.replay()
        torch.cuda.synchronize()
        _check(({"loss_cls": out[0].cpu(), "loss_box_reg": out[1].cpu()}, out[2].cpu(), out[3], out[4]), want,
               torch.bfloat16, "[replay]")
    assert all(torch.equal(a, b) for a, b in zip(out, eager[0]))  # back on the first inputs: the eager bits


def test_binding_against_the_reference_method():
    """`patch(only=["box_loss"])` rebinds FastRCNNOutputLayers.losses of the reference's own package; same inputs, same
    weights: losses and weight gradients against the unpatched method.  `patch()` without `only` leaves it alone."""
    try:
        import _reference_model as rm

        rm.install()
    except (RuntimeError, ImportError) as e:  # (no byte-compiled reference package on this checkout)
        pytest.skip(f"the reference's FastRCNNOutputLayers cannot be loaded: {e}")
    import detectron2
    from detectron2.layers import ShapeSpec
    from detectron2.modeling.box_regression import Box2BoxTransform
    from detectron2.modeling.roi_heads.fast_rcnn import FastRCNNOutputLayers
    from detectron2.structures import Boxes, Instances
    from detectron2.utils.events import EventStorage
    from detectron2_amd import integrate

    K, rows = 5, [40, 27]
    torch.manual_seed(0)
    layer = FastRCNNOutputLayers(ShapeSpec(channels=16), box2box_transform=Box2BoxTransform(weights=WEIGHTS),
                                 num_classes=K, smooth_l1_beta=0.5).to(DEV)
    _, _, classes, boxes, gt = _inputs(sum(rows), K, torch.float32, False, seed=4)
    classes[classes < 0] = K  # (the reference's cross_entropy has no padding rows)
    feats = torch.randn(sum(rows), 16, device=DEV)
    insts = []
    for c, b, t in zip(classes.split(rows), boxes.split(rows), gt.split(rows)):
        it = Instances((800, 800))
        it.proposal_boxes, it.gt_boxes, it.gt_classes = Boxes(b.to(DEV)), Boxes(t.to(DEV)), c.to(DEV)
        insts.append(it)

    def run():
        layer.zero_grad(set_to_none=True)
        with EventStorage(0):
            losses = layer.losses(layer(feats), insts)
        sum(losses.values()).backward()
        return ({k: float(v.detach()) for k, v in losses.items()},
                [layer.cls_score.weight.grad.clone(), layer.bbox_pred.weight.grad.clone()])

    original = FastRCNNOutputLayers.losses
    want_l, want_g = run()
    with integrate.patch(detectron2, layers=False):
        assert FastRCNNOutputLayers.losses is original
    with integrate.patch(detectron2, layers=False, only=["box_loss"]):
        assert FastRCNNOutputLayers.losses is not original
        got_l, got_g = run()
        assert layer._d2amd_box_loss_stats[0] == sum(rows)
    assert FastRCNNOutputLayers.losses is original
    print(got_l, want_l, [float((a - b).norm() / b.norm()) for a, b in zip(got_g, want_g)])
    assert set(got_l) == set(want_l) and all(abs(got_l[k] - want_l[k]) <= 1e-5 * abs(want_l[k]) for k in want_l)
    assert all((a - b).norm() <= 1e-4 * b.norm() for a, b in zip(got_g, want_g))
