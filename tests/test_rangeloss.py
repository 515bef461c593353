"""The range-view training criterion on the device (csrc/rangeloss.hip) against its contract,
rangeloss.range_criterion_host in float64 on the upcast logits. The yardstick of every bound is the same host form in float32,
the reference's own arithmetic on the same input:
  values    |device - host64| <= 4 max(|host32 - host64|, 2^-23 |host64|) per term;
  gradient  max |device - host64| <= max(4 max |host32 - host64|, 2^-22 max |host64|), plus half an ulp of a 16-bit output, both
            sides over the same elements: those that are one of the two smallest of a 3 x 3 window whose two smallest float64
            probabilities are within 1e-5 relative are left out (fp32 may pick the other pixel), at most 1e-3 of all elements.
On blocks of identical logit vectors the same gradient bound holds with NO mask: the tie rule is part of the contract.
The measured ratios (error / bound) of every case go to profiles/rangeloss_parity.json."""
import json
import os

import numpy as np
import pytest
import torch

import rangeloss_cases as rl
from openpcseg_amd import rangeloss

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY_JSON = os.path.join(ROOT, "profiles", "rangeloss_parity.json")
TERMS = ("ce", "dice", "ls", "bd")
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
# the gradient pass tiles 8 x 32 pixels up to 30 classes and 4 x 32 above; the statistics pass 8 x 32 always
SHAPES = [(1, 2, 1, 1), (1, 20, 1, 67), (2, 3, 70, 1), (1, 5, 19, 71), (2, 32, 11, 40)]
_HOST = {}


def _record_parity(key, value):
    data = {}
    if os.path.exists(PARITY_JSON):
        with open(PARITY_JSON) as f:
            data = json.load(f)
    data[key] = value
    try:
        with open(PARITY_JSON, "w") as f:
            json.dump(data, f, indent=1, sort_keys=True)
    except OSError:   # a read-only checkout: the figures are in the test's output
        pass


def _host_pair(key, logits, labels, **opts):
    """host64 and host32 of one input, computed once per key and left unchanged."""
    if key not in _HOST:
        _HOST[key] = (rl.host(logits, labels, torch.float64, **opts), rl.host(logits, labels, torch.float32, **opts))
    return _HOST[key]


def _device(logits, labels, grad_out=None, **opts):
    """RangeCriterion on the device -> (total, terms (4), grad) as float64 NumPy, and the raw device tensors."""
    dev = torch.device("cuda:0")
    crit = rangeloss.RangeCriterion(logits.shape[1], **opts).to(dev)
    x = logits.to(dev).requires_grad_(True)
    loss = crit(x, labels.to(dev))
    assert loss.dim() == 0 and loss.dtype == torch.float32 and crit.last_terms.is_cuda and crit.last_terms.shape == (4,)
    (grad,) = torch.autograd.grad(loss, x, grad_outputs=grad_out)
    assert grad.dtype == logits.dtype and grad.shape == logits.shape
    return (np.float64(loss.item()), crit.last_terms.double().cpu().numpy(), grad.double().cpu().numpy()), (loss, crit.last_terms, grad)


def _check(name, logits, labels, dtype=torch.float32, use_mask=True, **opts):
    """The value and gradient bounds of the module docstring for one case; records and returns the ratios."""
    logits = logits.to(dtype)
    (t64, terms64, g64), (t32, terms32, g32) = _host_pair(name, logits.float(), labels, **opts)
    (total, terms, grad), _ = _device(logits, labels, **opts)
    ratios = {k: rl.value_ratio(terms[i], terms64[i], terms32[i]) for i, k in enumerate(TERMS)}
    ratios["total"] = rl.value_ratio(total, t64, t32)
    mask = rl.close_mask(logits.float()) if use_mask else None
    share = float(mask.mean()) if mask is not None else 0.0
    ratios["grad"] = rl.grad_ratio(grad, g64, g32, dtype, mask)
    ratios["masked_share"] = share
    print(name, {k: float("%.3g" % v) for k, v in ratios.items()}, "terms", terms, "host64", terms64)
    _record_parity(name, ratios)
    assert share <= rl.MASK_CAP, (name, share)
    for k in TERMS + ("total", "grad"):
        assert ratios[k] <= 1.0, (name, k, ratios[k], terms, terms64, terms32)
    return ratios


@pytest.fixture(scope="module")
def gold():
    return rl.load_gold()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_edge_shapes(shape):
    logits, labels = rl.make_logits(shape, sum(shape)), rl.make_labels(shape, sum(shape))
    ratios = _check("shape_" + "x".join(map(str, shape)), logits, labels)
    if shape == (1, 2, 1, 1):   # the window is the pixel itself: the boundary term is exactly 1
        (_, terms, grad), _ = _device(logits, labels)
        assert terms[3] == 1.0
        (_, _, g_off), _ = _device(logits, labels, boundary=False)
        assert np.array_equal(grad, g_off)   # and its gradient exactly 0
    assert ratios["masked_share"] <= rl.MASK_CAP


@pytest.mark.parametrize("case", [0, 1])
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_fixture_inputs(gold, case, dtype):
    logits, labels = rl.gold_case(gold, case)
    ratios = _check("fixture%d_%s" % (case, dtype), logits, labels, DTYPES[dtype])
    if dtype == "fp32":
        assert ratios["masked_share"] == 0.0   # the generator's seed guard
        (total, terms, grad), _ = _device(logits, labels)
        g64 = gold["c%d_grad64" % case]
        g32 = rl.gold_grad32(gold, case).astype(np.float64)
        assert rl.grad_ratio(grad, g64, g32) <= 1.0                                   # the reference's own records
        rec = lambda k, b: float(gold["c%d_%s%d" % (case, k, b)].reshape(-1)[0])
        for k, v in (("ls", terms[2]), ("bd", terms[3]), ("total", total), ("ced", terms[0] + terms[1])):
            bound = 4 * max(abs(rec(k, 32) - rec(k, 64)), 2.0 ** -23 * abs(rec(k, 64)))   # ced: the sum of two positive terms
            assert abs(v - rec(k, 64)) <= bound, (k, v, rec(k, 64), rec(k, 32))


@pytest.mark.parametrize("kind", ["absent", "image0", "all0"])
def test_label_cases(kind):
    shape = (3, 20, 9, 70)
    logits, labels = rl.make_logits(shape, 7), rl.make_labels(shape, 7, kind)
    _check("labels_" + kind, logits, labels)
    if kind == "all0":   # Lovasz takes its "no class present" branch
        (_, terms, _), _ = _device(logits, labels)
        assert terms[2] == 0.0


def test_out_of_range_labels():
    shape = (2, 6, 9, 40)
    logits, labels = rl.make_logits(shape, 8), rl.make_labels(shape, 8)
    labels[0, 2:5, 3:20] = 6
    labels[1, 0, 0] = -1
    labels[1, 8, 39] = 255
    _check("labels_out_of_range", logits, labels)


@pytest.mark.parametrize("opts", [
    {"lovasz": False}, {"boundary": False}, {"lovasz": False, "boundary": False}, {"weights": (0.7, 2.0, 1.5)},
    {"loss": "wce"}, {"loss": "wce", "class_weight": "semkitti"}], ids=lambda o: "-".join("%s=%s" % kv for kv in o.items()).replace(" ", ""))
def test_options(gold, opts):
    logits, labels = rl.gold_case(gold, 0)
    opts = dict(opts)
    if opts.get("class_weight") == "semkitti":
        opts["class_weight"] = [float(v) for v in gold["semkitti_weight"]]
    _check("options_" + "_".join(sorted(opts)) + ("_cw" if "class_weight" in opts else ""), logits, labels, **opts)


def test_channels_last_and_four_dim_labels(gold):
    logits, labels = rl.gold_case(gold, 1)
    (t_a, terms_a, g_a), _ = _device(logits, labels)
    dev = torch.device("cuda:0")
    x = logits.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    assert not x.is_contiguous()
    crit = rangeloss.RangeCriterion(17)
    loss = crit(x, labels.to(dev).unsqueeze(1))
    (g,) = torch.autograd.grad(loss, x)
    assert loss.item() == t_a and np.array_equal(g.double().cpu().numpy(), g_a)


def test_ties_need_no_mask():
    """Blocks of identical logit vectors: a kernel that split or misplaced the tie gradient would be off by whole coefficients."""
    for shape, seed in (((2, 5, 19, 45), 3), ((1, 30, 9, 37), 4)):
        logits, labels = rl.tie_logits(shape, seed), rl.make_labels(shape, seed, block=(3, 4))
        _check("ties_" + "x".join(map(str, shape)), logits, labels, use_mask=False)


def test_full_width_image_once():
    shape = (1, 20, 64, 512)
    logits, labels = rl.make_logits(shape, 9), rl.make_labels(shape, 9, block=(5, 23))
    _check("shape_1x20x64x512", logits, labels)


def test_two_calls_are_bit_identical(gold):
    logits, labels = rl.gold_case(gold, 0)
    for dtype in (torch.float32, torch.bfloat16):
        _, (l1, t1, g1) = _device(logits.to(dtype), labels)
        _, (l2, t2, g2) = _device(logits.to(dtype), labels)
        assert torch.equal(l1, l2) and torch.equal(t1, t2) and torch.equal(g1, g2)


def test_autograd_scales_the_gradient_pass(gold):
    logits, labels = rl.gold_case(gold, 1)
    _, (_, _, g1) = _device(logits, labels)
    _, (_, _, g3) = _device(logits, labels, grad_out=torch.tensor(-2.5, device="cuda:0"))
    assert torch.equal(g3, g1 * -2.5)
    dev = torch.device("cuda:0")
    x = logits.to(dev).requires_grad_(True)
    (rangeloss.RangeCriterion(17)(x * 2.0, labels.to(dev)) * 0.5).backward()      # through a graph on both sides
    assert torch.allclose(x.grad, rangeloss_grad_at(logits * 2.0, labels), rtol=1e-6, atol=0)
    want = _device(logits, labels)[0][0]
    with torch.no_grad():                                                          # no gradient wanted: value only
        assert rangeloss.RangeCriterion(17)(logits.to(dev), labels.to(dev)).item() == want


def rangeloss_grad_at(logits, labels):
    _, (_, _, g) = _device(logits, labels)
    return g


def test_environment_switch_gives_the_fallback(gold, monkeypatch):
    logits, labels = rl.gold_case(gold, 0)
    (t64, terms64, _), (t32, terms32, _) = _host_pair("fixture0_fp32", logits, labels)
    monkeypatch.setenv("PCS_RANGE_LOSS", "0")
    dev = torch.device("cuda:0")
    crit = rangeloss.RangeCriterion(20)
    x = logits.to(dev).requires_grad_(True)
    assert not crit.uses_kernel(x)
    loss = crit(x, labels.to(dev))
    loss.backward()
    assert rl.value_ratio(loss.item(), t64, t32) <= 1.0
    for i in range(4):
        assert rl.value_ratio(crit.last_terms[i].item(), terms64[i], terms32[i]) <= 1.0, TERMS[i]
    assert torch.isfinite(x.grad).all()


def test_cenet_heads_on_the_device(gold):
    logits, labels = rl.gold_case(gold, 1)
    dev = torch.device("cuda:0")
    heads = [(logits * s).to(dev).requires_grad_(True) for s in (1.0, 0.5, 0.25, 0.125)]
    crit = rangeloss.RangeCriterion(17)
    loss = rangeloss.cenet_criterion(crit, heads[0], heads[1:], labels.to(dev))
    singles = [_device(logits * s, labels)[0][0] for s in (1.0, 0.5, 0.25, 0.125)]
    want = 1.25 * singles[0] + singles[1] + singles[2] + singles[3]
    assert abs(loss.item() - want) <= 1e-6 * abs(want)
    grads = torch.autograd.grad(loss, heads)
    assert torch.equal(grads[1], rangeloss_grad_at(logits * 0.5, labels))
