"""The range-view training criterion on the host: rangeloss.range_criterion_host reproduces
tests/golden/rangeloss_golden.npz -- the output of RUNNING the reference's CrossEntropyDiceLoss, Lovasz_softmax and BoundaryLoss
(tests/golden/make_rangeloss_golden.py) -- in both precisions; the tie rule and the label extension hold on constructed data; the
fallback and the CENet combination equal their literal forms; the new C entries are declared, exported and refuse bad sizes
without a device."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import rangeloss_cases as rl
from openpcseg_amd import native, rangeloss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("pcs_range_loss_ws_bytes", "pcs_range_loss_stats", "pcs_range_loss_fold", "pcs_range_loss_grad")


@pytest.fixture(scope="module")
def gold():
    return rl.load_gold()


def _records(gold, i, bits):
    pre = "c%d_" % i
    return {k: float(gold["%s%s%d" % (pre, k, bits)].reshape(-1)[0]) for k in ("ced", "ls", "bd", "total")}


def _host_terms(logits, labels, dtype, weights):
    """total, ls, bd of the full criterion, and ced = mean(CE + Dice) as the reference forms it: the total with the other terms off."""
    total, (_, _, ls, bd), grad = rl.host(logits, labels, dtype, weights=weights)
    ced = rl.host(logits, labels, dtype, weights=(1.0, 0.0, 0.0), lovasz=False, boundary=False)[0]
    return {"ced": ced, "ls": ls, "bd": bd, "total": total}, grad


@pytest.mark.parametrize("case", [0, 1])
def test_float64_host_form_reproduces_the_reference(gold, case):
    """The same operations in the same order: only a BLAS-free summation order can differ."""
    logits, labels = rl.gold_case(gold, case)
    got, grad = _host_terms(logits, labels, torch.float64, tuple(gold["weights"]))
    rec = _records(gold, case, 64)
    for name, a in got.items():
        assert abs(a - rec[name]) <= 1e-10 * abs(rec[name]), (name, a, rec[name])
    g64 = gold["c%d_grad64" % case]
    assert np.abs(grad - g64).max() <= 1e-10 * np.abs(g64).max()


@pytest.mark.parametrize("case", [0, 1])
def test_float32_host_form_reproduces_the_float32_record(gold, case):
    """To the float32 distance the fixture itself shows between its two precisions, times 4."""
    logits, labels = rl.gold_case(gold, case)
    got, grad = _host_terms(logits, labels, torch.float32, tuple(gold["weights"]))
    r64, r32 = _records(gold, case, 64), _records(gold, case, 32)
    for name, a in got.items():
        assert abs(a - r32[name]) <= 4 * abs(r32[name] - r64[name]), (name, a, r32[name], r64[name])
    g64, g32 = gold["c%d_grad64" % case], rl.gold_grad32(gold, case).astype(np.float64)
    assert np.abs(grad - g32).max() <= 4 * np.abs(g32 - g64).max()


def test_fixture_inputs_are_what_the_issue_asks(gold):
    assert [tuple(s) for s in gold["shapes"]] == [(2, 20, 9, 70), (3, 17, 5, 33)]
    for i in range(2):
        logits, labels = rl.gold_case(gold, i)
        assert (labels == 0).any() and len(torch.unique(labels[-1])) <= 4 < len(torch.unique(labels))   # class 0, absent classes
        assert not rl.close_mask(logits).any()                                                         # the seed guard
    assert gold["semkitti_weight"].shape == (20,) and gold["semkitti_weight"][0] == 0.0


def test_tie_rule_on_constructed_data():
    """An all-equal 4 x 5 image: torch's max_pool2d backward gives the whole gradient of every window to the first element in
    row-major order of the clipped window -- the rule the kernel's contract names. Element (0, 0) is the first of 4 windows."""
    x = torch.zeros(1, 1, 4, 5, dtype=torch.float64, requires_grad=True)
    F.max_pool2d(1 - x, 3, 1, 1).sum().backward()
    g = -x.grad[0, 0]
    assert g[0, 0] == 4 and g.sum() == 20 and g[3, 4] == 0 and g[1, 1] == 1 and g[0, 1] == 2 and g[1, 0] == 2
    # and through the whole host form on blocks of identical logit vectors: float32 and float64 pick the same elements
    shape = (2, 5, 7, 11)
    logits, labels = rl.tie_logits(shape, 5), rl.make_labels(shape, 5, block=(3, 4))
    _, t64, g64 = rl.host(logits, labels, torch.float64)
    _, t32, g32 = rl.host(logits, labels, torch.float32)
    assert np.abs(g32 - g64).max() <= 1e-5 * np.abs(g64).max() and np.abs(t32 - t64).max() <= 1e-5


def test_out_of_range_labels_are_ignored_pixels():
    shape = (2, 6, 5, 9)
    logits, labels = rl.make_logits(shape, 21), rl.make_labels(shape, 21, block=(2, 3))
    bad = labels.clone()
    bad[0, 1:3, 2:5] = 6
    bad[1, 0, 0] = -1
    bad[1, 4, 8] = 255
    total, (ce, dice, ls, bd), grad = rl.host(logits, bad, torch.float64)
    x = logits.double()
    invalid = (bad < 0) | (bad >= 6)
    logp = F.log_softmax(x, dim=1)
    picked = logp.gather(1, bad.clamp(0, 5).unsqueeze(1)).squeeze(1)
    assert abs(ce - float((-picked * ~invalid).sum() / invalid.numel())) <= 1e-12       # term 0, still in the divisor
    p = F.softmax(x, dim=1)
    onehot = F.one_hot(bad.clamp(0, 5), 6).permute(0, 3, 1, 2).double() * (~invalid).unsqueeze(1)
    inter = (p * onehot).sum((0, 2, 3))
    den = ((p + onehot) * (~invalid).unsqueeze(1)).sum((0, 2, 3)) + 1e-4                # left out of the denominator
    assert abs(dice - float((1 - 2 * inter / den).sum() / 6)) <= 1e-12
    assert np.isfinite(grad).all() and np.isfinite([total, ls, bd]).all()
    # every pixel invalid: the reference's "only void" branch -- Dice and CE are zero
    _, (ce0, dice0, ls0, _), _ = rl.host(logits, torch.full_like(labels, 99), torch.float64)
    assert ce0 == 0 and dice0 == 0 and ls0 == 0


def test_top_k_goes_through_the_fallback_and_equals_the_literal_form():
    shape = (2, 7, 6, 10)
    logits, labels = rl.make_logits(shape, 31), rl.make_labels(shape, 31, block=(2, 3))
    crit = rangeloss.RangeCriterion(7, top_k_percent_pixels=0.3)
    assert not crit.uses_kernel(logits)
    x = logits.clone().requires_grad_(True)
    loss = crit(x, labels.unsqueeze(1))                        # (B, 1, H, W) labels are squeezed as the models do
    loss.backward()
    y = logits.clone().requires_grad_(True)
    p = F.softmax(y, dim=1)
    pixel = (F.cross_entropy(y, labels, reduction="none") + rangeloss._dice_loss_multichannel(p, labels)).view(-1)
    top, _ = torch.topk(pixel, int(0.3 * pixel.numel()))
    from openpcseg_amd.workloads.losses import lovasz_softmax_per_class
    literal = (top.mean() + 3.0 * lovasz_softmax_per_class(p.permute(0, 2, 3, 1).reshape(-1, 7), labels.view(-1), ignore=0) +
               rangeloss._boundary_loss(p, labels, torch.ones_like(labels, dtype=torch.bool)))
    literal.backward()
    assert abs(loss.item() - literal.item()) <= 1e-5 * abs(literal.item())
    assert (x.grad - y.grad).abs().max() <= 1e-5 * y.grad.abs().max()
    assert crit.last_terms.shape == (4,)
    with pytest.raises(ValueError):
        rangeloss.RangeCriterion(7, loss="dice", class_weight=[1.0] * 7)
    with pytest.raises(ValueError):
        rangeloss.RangeCriterion(7, loss="focal")


def test_wce_is_the_weighted_cross_entropy(gold):
    logits, labels = rl.gold_case(gold, 0)
    w = torch.from_numpy(gold["semkitti_weight"])
    total, (ce, dice, ls, bd), _ = rl.host(logits, labels, torch.float64, loss="wce", class_weight=w, lovasz=False, boundary=False)
    want = F.cross_entropy(logits.double(), labels, weight=w, reduction="none").mean().item()
    assert abs(ce - want) <= 1e-12 and dice == 0 and ls == 0 and bd == 0 and abs(total - want) <= 1e-12


def test_cenet_criterion_equals_the_literal_sum():
    shape = (2, 5, 6, 9)
    labels = rl.make_labels(shape, 41, block=(2, 3))
    heads = [rl.make_logits(shape, 41 + i).requires_grad_(True) for i in range(4)]
    crit = rangeloss.RangeCriterion(5)
    loss = rangeloss.cenet_criterion(crit, heads[0], heads[1:], labels)
    terms = crit.last_terms.clone()
    singles = []
    for head in heads:
        singles.append((crit(head, labels), crit.last_terms.clone()))
    literal = 1.25 * singles[0][0] + singles[1][0] + singles[2][0] + singles[3][0]
    assert abs(loss.item() - literal.item()) <= 1e-6 * abs(literal.item())
    literal_terms = 1.25 * singles[0][1] + singles[1][1] + singles[2][1] + singles[3][1]
    assert torch.allclose(terms, literal_terms, rtol=1e-6, atol=0)
    ce, dice, ls, bd = terms.tolist()
    assert abs(loss.item() - (1.0 * (ce + dice) + 3.0 * ls + 1.0 * bd)) <= 1e-5 * abs(loss.item())   # cenet.py:266-288
    grads = torch.autograd.grad(loss, heads)
    assert all(torch.isfinite(g).all() and g.abs().max() > 0 for g in grads)


def test_new_entries_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "pcseg_hip.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    for decl in (
            "int64_t pcs_range_loss_ws_bytes(int32_t B, int32_t C, int32_t H, int32_t W);",
            "int pcs_range_loss_stats(const void *logits, int32_t dtype, const int64_t *labels, const float *class_weight, int32_t B, "
            "int32_t C, int32_t H, int32_t W, int32_t flags, float *probas, void *ws, int64_t ws_bytes, void *stream);",
            "int pcs_range_loss_fold(int32_t B, int32_t C, int32_t H, int32_t W, int32_t flags, const float *lovasz, float w_ce, "
            "float w_ls, float w_bd, float *terms, void *ws, int64_t ws_bytes, void *stream);",
            "int pcs_range_loss_grad(const void *logits, int32_t dtype, const int64_t *labels, const float *class_weight, "
            "const float *lovasz_grad, int32_t B, int32_t C, int32_t H, int32_t W, int32_t flags, float w_ce, float w_ls, "
            "const void *ws, int64_t ws_bytes, void *grad, void *stream);"):
        assert decl in flat, decl
    assert re.search(r"#define PCS_ABI_VERSION 12\b", hdr)
    assert re.search(r"#define PCS_RANGE_LOSS_DICE 1\b", hdr) and re.search(r"#define PCS_RANGE_LOSS_BOUNDARY 2\b", hdr)
    lib = native.load_library()   # dlopen works without a GPU
    for name in ENTRIES:
        assert name in native.SIGNATURES and hasattr(lib, name), name
    assert lib.pcs_abi_version() == native.ABI_VERSION == 12
    assert hasattr(native.HipBackend, "range_loss_stats") and hasattr(native.HipBackend, "range_loss_grad")


def test_size_only_refusals():
    """Sizes are checked before any pointer is looked at, so the refusals need no device."""
    lib = native.load_library()
    assert lib.pcs_range_loss_ws_bytes(30, 20, 64, 512) > 0 and lib.pcs_range_loss_ws_bytes(1, 2, 1, 1) > 0
    assert lib.pcs_range_loss_ws_bytes(12, 32, 64, 2048) > 0
    bad = ((0, 20, 64, 512), (-1, 20, 64, 512), (1, 1, 64, 512), (1, 33, 64, 512), (1, 20, 0, 512), (1, 20, 64, 0),
           (1, 20, 64, -4), (64, 32, 1024, 2048), (1, 2, 46341, 46341))   # the last two: B C H W >= 2^32 - 1
    for b, c, h, w in bad:
        assert lib.pcs_range_loss_ws_bytes(b, c, h, w) == -1 and b"pcs_range_loss_ws_bytes" in lib.pcs_last_error(), (b, c, h, w)
        assert lib.pcs_range_loss_stats(None, 0, None, None, b, c, h, w, 3, None, None, 0, None) == -1
        assert b"pcs_range_loss_stats" in lib.pcs_last_error()
        assert lib.pcs_range_loss_fold(b, c, h, w, 3, None, 1.0, 3.0, 1.0, None, None, 0, None) == -1
        assert lib.pcs_range_loss_grad(None, 0, None, None, None, b, c, h, w, 3, 1.0, 3.0, None, 0, None, None) == -1
        assert b"pcs_range_loss_grad" in lib.pcs_last_error()
    assert lib.pcs_range_loss_stats(None, 3, None, None, 1, 20, 8, 8, 3, None, None, 0, None) == -1 and b"dtype" in lib.pcs_last_error()
    assert lib.pcs_range_loss_stats(None, 0, None, None, 1, 20, 8, 8, 4, None, None, 0, None) == -1 and b"flags" in lib.pcs_last_error()
    assert lib.pcs_range_loss_stats(None, 0, None, None, 1, 20, 8, 8, 3, None, None, 0, None) == -1
    assert b"null pointer" in lib.pcs_last_error()
    assert lib.pcs_range_loss_grad(None, 2, None, None, None, 1, 20, 8, 8, 3, 1.0, 3.0, None, 0, None, None) == -1
    assert b"null pointer" in lib.pcs_last_error()
