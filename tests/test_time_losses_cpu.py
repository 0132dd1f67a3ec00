"""Host-side checks of the time-domain losses (losses.time_domain_loss, ESRLoss .. SDSDRLoss, FIRFilter; csrc/tdloss.hip): option
validation, the modules' auraloss signatures, the C ABI's argument checks without a device, and the float64 restatement
(tests/auraloss_time_restated.py) against closed forms written out by hand."""
import inspect
import math

import pytest
import torch

from dasp_pytorch_amd import _lib, losses
from tests import auraloss_time_restated as R

X = torch.zeros(2, 1, 8)


def test_unknown_keyword_and_positional_weights_are_refused():
    with pytest.raises(TypeError, match="w_l1"):
        losses.time_domain_loss(X, X, w_l1=1.0)
    with pytest.raises(TypeError):
        losses.time_domain_loss(X, X, 1.0)                      # the weights are keyword-only


def test_all_weights_zero():
    with pytest.raises(ValueError, match="non-zero"):
        losses.time_domain_loss(X, X)
    with pytest.raises(ValueError, match="non-zero"):
        losses.time_domain_loss(X, X, w_esr=0.0, w_mse=0.0)


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_non_finite_options(bad):
    with pytest.raises(ValueError, match="finite"):
        losses.time_domain_loss(X, X, w_esr=1.0, w_dc=bad)
    with pytest.raises(ValueError, match="eps"):
        losses.time_domain_loss(X, X, w_esr=1.0, eps=bad)
    with pytest.raises(ValueError, match="a must be positive"):
        losses.time_domain_loss(X, X, w_log_cosh=1.0, a=bad)


@pytest.mark.parametrize("a", [0.0, -1.0])
def test_a_must_be_positive(a):
    with pytest.raises(ValueError, match="a must be positive"):
        losses.time_domain_loss(X, X, w_log_cosh=1.0, a=a)
    with pytest.raises(ValueError, match="a must be positive"):
        losses.LogCoshLoss(a=a)


def test_bad_reduction():
    with pytest.raises(ValueError, match="reduction"):
        losses.time_domain_loss(X, X, w_esr=1.0, reduction="batchmean")
    with pytest.raises(ValueError, match="reduction"):
        losses.ESRLoss(reduction=None)


def test_shape_mismatch_and_empty_input():
    with pytest.raises(RuntimeError, match="same shape"):
        losses.time_domain_loss(X, torch.zeros(2, 1, 9), w_esr=1.0)
    with pytest.raises(RuntimeError, match="same shape"):
        losses.ESRLoss()(X, torch.zeros(1, 2, 8))
    with pytest.raises(RuntimeError, match="same shape"):
        losses.FIRFilter()(X, torch.zeros(2, 1, 9))
    with pytest.raises(ValueError, match="at least one sample"):
        losses.time_domain_loss(torch.zeros(2, 0), torch.zeros(2, 0), w_esr=1.0)


def test_no_cpu_path():
    with pytest.raises(_lib.DaspHipError):
        losses.time_domain_loss(X, X, w_esr=1.0)
    with pytest.raises(_lib.DaspHipError):
        losses.FIRFilter("hp")(X, X)


def test_fir_filter_options():
    with pytest.raises(ValueError, match="odd"):
        losses.FIRFilter("hp", ntaps=100)
    with pytest.raises(ValueError, match="filter_type"):
        losses.FIRFilter("lp")
    with pytest.raises(NotImplementedError, match="101"):
        losses.FIRFilter("aw", ntaps=51)
    f = losses.FIRFilter()
    assert (f.filter_type, f.coef, f.fs, f.ntaps) == ("hp", 0.85, 44100, 101)
    assert f._taps.tolist() == pytest.approx([1.0, -0.85, 0.0])
    assert losses.FIRFilter("fd", 0.5)._taps.tolist() == [1.0, 0.0, -0.5]
    assert losses.FIRFilter("aw", fs=48000)._taps is losses.a_weighting_taps(48000.0)


SIGNATURES = {
    "ESRLoss": (("eps", 1e-8), ("reduction", "mean")),
    "DCLoss": (("eps", 1e-8), ("reduction", "mean")),
    "LogCoshLoss": (("a", 1.0), ("eps", 1e-8), ("reduction", "mean")),
    "SNRLoss": (("zero_mean", True), ("eps", 1e-8), ("reduction", "mean")),
    "SISDRLoss": (("zero_mean", True), ("eps", 1e-8), ("reduction", "mean")),
    "SDSDRLoss": (("zero_mean", True), ("eps", 1e-8), ("reduction", "mean")),
}
TERM = {"ESRLoss": 0, "DCLoss": 1, "LogCoshLoss": 2, "SNRLoss": 3, "SISDRLoss": 4, "SDSDRLoss": 5}


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_constructor_defaults_and_positional_order(name):
    cls = getattr(losses, name)
    params = list(inspect.signature(cls.__init__).parameters.values())[1:]
    assert tuple((p.name, p.default) for p in params) == SIGNATURES[name]
    assert all(p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for p in params)
    w, a, eps, zero_mean, red = cls()._cfg
    assert w == tuple(1.0 if k == TERM[name] else 0.0 for k in range(7)) and (a, eps, zero_mean, red) == (1.0, 1e-8, True, 1)
    # positional = keyword
    other = {"a": 2.5, "zero_mean": False, "eps": 1e-5, "reduction": "sum"}
    args = [other[p.name] for p in params]
    assert cls(*args)._cfg == cls(**{p.name: other[p.name] for p in params})._cfg
    w, a, eps, zero_mean, red = cls(*args)._cfg
    assert eps == 1e-5 and red == 2
    assert a == (2.5 if name == "LogCoshLoss" else 1.0)
    assert zero_mean is (name not in ("SNRLoss", "SISDRLoss", "SDSDRLoss"))


def test_functional_signature():
    sig = inspect.signature(losses.time_domain_loss)
    kw = [(p.name, p.default) for p in sig.parameters.values() if p.kind is inspect.Parameter.KEYWORD_ONLY]
    assert kw == [("w_esr", 0.0), ("w_dc", 0.0), ("w_log_cosh", 0.0), ("w_snr", 0.0), ("w_si_sdr", 0.0), ("w_sd_sdr", 0.0), ("w_mse", 0.0),
                  ("a", 1.0), ("zero_mean", True), ("eps", 1e-8), ("reduction", "mean")]


# ---- the C ABI without a device ------------------------------------------------------------------------------------------------------
W1 = (1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)


def test_scratch_size_query():
    L = _lib.lib()
    q = L.dasp_tdloss_scratch_doubles
    assert q(0, 16) == -1 and q(1, 0) == -1 and q(-3, 16) == -1
    # per (row, segment) six sums, per row one fp64 loss; short rows are one segment
    assert q(1, 1) == 7 and q(33, 257) == 33 * 7 and q(6, 4096) == 6 * 7
    assert q(6, 4099) == 6 * (2 * 6 + 1)                                    # segments of at least 4096 samples: a 3-sample second one
    assert q(1, 70001) == 18 * 6 + 1
    assert q(32, 131072) == 32 * (32 * 6 + 1)                               # few rows: 32 x 32 = 1024 workgroups
    assert q(512, 131072) == 512 * (2 * 6 + 1)                              # many rows are not over-split: 1024 workgroups again
    assert q(4096, 131072) == 4096 * 7                                      # one workgroup per row
    assert q(1 << 31, 16) == -1                                             # more workgroups than a grid has


def test_abi_argument_checks_without_gpu():
    """NULL pointers, rows or N < 1 and bad options are DASP_ERR_ARG (-1) before anything touches the device; sizes the plan cannot take
    are DASP_ERR_UNSUPPORTED (-2). The pointers are never dereferenced on the host."""
    L = _lib.lib()
    fwd, bwd = L.dasp_tdloss_forward, L.dasp_tdloss_backward
    ok = (8, 8, 8, 8, 8, 8)
    tail = (1.0, 1e-8, 1, 1, None)
    for k in range(5):                                                      # pred, target, scratch, moments, row_loss
        ptrs = list(ok)
        ptrs[k] = None
        assert fwd(*ptrs, 2, 16, *W1, *tail) == -1, k
    assert fwd(8, 8, 8, 8, 8, None, 2, 16, *W1, *tail) == -1                # reduction = mean needs the scalar
    assert fwd(*ok, 0, 16, *W1, *tail) == -1 and fwd(*ok, 2, 0, *W1, *tail) == -1 and fwd(*ok, -1, 16, *W1, *tail) == -1
    assert fwd(*ok, 2, 16, *([0.0] * 7), *tail) == -1                       # no term
    assert fwd(*ok, 2, 16, 1.0, float("nan"), 0.0, 0.0, 0.0, 0.0, 0.0, *tail) == -1
    assert fwd(*ok, 2, 16, 0.0, 0.0, 0.0, 0.0, float("inf"), 0.0, 0.0, *tail) == -1
    assert fwd(*ok, 2, 16, *W1, 0.0, 1e-8, 1, 1, None) == -1 and fwd(*ok, 2, 16, *W1, -1.0, 1e-8, 1, 1, None) == -1      # a <= 0
    assert fwd(*ok, 2, 16, *W1, 1.0, float("nan"), 1, 1, None) == -1        # eps
    assert fwd(*ok, 2, 16, *W1, 1.0, 1e-8, 1, 3, None) == -1 and fwd(*ok, 2, 16, *W1, 1.0, 1e-8, 1, -1, None) == -1      # reduction
    assert fwd(*ok, 1 << 31, 16, *W1, *tail) == -2
    for k in range(4):                                                      # pred, target, moments, gloss
        ptrs = list(ok)
        ptrs[k] = None
        assert bwd(*ptrs, 2, 16, *W1, *tail) == -1, k
    assert bwd(8, 8, 8, 8, None, None, 2, 16, *W1, *tail) == -1             # neither gradient asked for
    assert bwd(*ok, 0, 16, *W1, *tail) == -1 and bwd(*ok, 2, 0, *W1, *tail) == -1
    assert bwd(*ok, 2, 16, *([0.0] * 7), *tail) == -1
    assert bwd(*ok, 2, 16, *W1, 0.0, 1e-8, 1, 1, None) == -1
    assert bwd(*ok, 2, 16, *W1, 1.0, 1e-8, 1, 7, None) == -1
    assert bwd(*ok, 1 << 31, 16, *W1, *tail) == -2


# ---- the restatement against closed forms ---------------------------------------------------------------------------------------------
P = torch.tensor([[1.0, 2.0, 4.0, 1.0]], dtype=torch.float64)          # d = p - t = (0, 2, 1, 1): sum d = 4, sum d^2 = 6
T = torch.tensor([[1.0, 0.0, 3.0, 0.0]], dtype=torch.float64)          # sum t = 4, sum t^2 = 10, sum d t = 3, sum p t = 13, sum p^2 = 22


def db(x):
    return -10.0 * math.log10(x)


def test_restated_esr_dc_mse_log_cosh_by_hand():
    assert float(R.esr(P, T, eps=0.5)) == pytest.approx(6 / 10.5, rel=1e-14)
    assert float(R.dc(P, T, eps=0.5)) == pytest.approx(1.0 / (2.5 + 0.5), rel=1e-14)            # mean d = 1, mean t^2 = 2.5
    assert float(R.mse(P, T)) == pytest.approx(1.5, rel=1e-14)
    want = (math.log(1.0 + 0.25) + math.log(math.cosh(4.0) + 0.25) + 2 * math.log(math.cosh(2.0) + 0.25)) / 2.0 / 4.0
    assert float(R.log_cosh(P, T, a=2.0, eps=0.25)) == pytest.approx(want, rel=1e-14)


def test_restated_db_losses_by_hand():
    e = 0.5
    # as they are: E = 6, T = 10, alpha = 13 / 10.5
    assert float(R.snr(P, T, zero_mean=False, eps=e)) == pytest.approx(db(10 / 6.5 + e), rel=1e-14)
    al = 13 / 10.5
    num = al * al * 10
    res = 22 - 2 * al * 13 + num                                            # sum (p - alpha t)^2
    assert float(R.si_sdr(P, T, zero_mean=False, eps=e)) == pytest.approx(db(num / (res + e) + e), rel=1e-13)
    assert float(R.sd_sdr(P, T, zero_mean=False, eps=e)) == pytest.approx(db(num / 6.5 + e), rel=1e-13)
    # zero mean: p' = (-1, 0, 2, -1), t' = (0, -1, 2, -1): sum t'^2 = 6, sum (p' - t')^2 = 2, sum p' t' = 5
    assert float(R.snr(P, T, zero_mean=True, eps=e)) == pytest.approx(db(6 / 2.5 + e), rel=1e-14)
    al = 5 / 6.5
    num = al * al * 6
    res = 6 - 2 * al * 5 + num                                              # sum p'^2 = 6
    assert float(R.si_sdr(P, T, zero_mean=True, eps=e)) == pytest.approx(db(num / (res + e) + e), rel=1e-13)
    assert float(R.sd_sdr(P, T, zero_mean=True, eps=e)) == pytest.approx(db(num / 2.5 + e), rel=1e-13)


def test_restated_reductions_weights_and_mse_equals_torch():
    g = torch.Generator().manual_seed(0)
    p, t = torch.randn(3, 2, 50, generator=g, dtype=torch.float64), torch.randn(3, 2, 50, generator=g, dtype=torch.float64)
    rows = R.rows_loss(p, t, {"esr": 1.0, "dc": 1.0, "mse": 100.0, "snr": 0.0})
    assert rows.shape == (3, 2)
    assert torch.allclose(rows, R.esr(p, t) + R.dc(p, t) + 100 * R.mse(p, t), rtol=1e-14)
    assert float(R.reduce(rows, "mean")) == pytest.approx(float(rows.sum()) / 6) and float(R.reduce(rows, "sum")) == pytest.approx(float(rows.sum()))
    assert float(R.reduce(R.mse(p, t), "mean")) == pytest.approx(float(torch.nn.MSELoss()(p, t)), rel=1e-14)
    loss, gp, gt = R.loss_and_grads(p.numpy(), t.numpy(), {"mse": 1.0})
    assert gp == pytest.approx((2 * (p - t) / 300).numpy(), rel=1e-12) and gt == pytest.approx(-gp, rel=1e-12)
