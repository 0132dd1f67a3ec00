"""Host-side checks of resample (no GPU): the restatement (tests/resample_restated.py) against a plain double loop whose gradient is
written by hand, signal.resample_taps against an independent evaluation of the formula and the zero rule, the output lengths, the
transposed tables that the backward kernel gathers through, the size queries and argument checks of the C ABI, the errors of the Python
layer, modules.Resample, and the alias rejection of the default design (recorded, not bounded)."""
import inspect
import math

import numpy as np
import pytest
import torch

import dasp_pytorch_amd as D
from dasp_pytorch_amd import _lib, _resample_design
from tests import resample_restated as R
from tests.util import record

HANN = dict(resampling_method="sinc_interp_hann")
KAISER = dict(resampling_method="sinc_interp_kaiser")


def peak_err(a, b):
    return np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-300)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [HANN, KAISER], ids=["hann", "kaiser"])
@pytest.mark.parametrize("o,n,N", [(2, 3, 41), (3, 2, 41), (147, 160, 300), (441, 160, 900)])
def test_restatement_equals_the_double_loop(o, n, N, kw):
    """Both in float64 on the same float32 taps: rounding only, 1e-13 of the peak (at most 53 products per output). The adjoint of the
    restatement itself holds to 1e-13 as well."""
    g = torch.Generator().manual_seed(o + n)
    x = torch.randn(2, N, generator=g, dtype=torch.float64)
    M = R.out_len(o, n, N)
    w = torch.randn(2, M, generator=g, dtype=torch.float64)
    a, b = R.forward_backward(x, w, o, n, **kw), R.direct(x.numpy(), w.numpy(), o, n, **kw)
    for k in ("y", "gx"):
        assert a[k].shape == b[k].shape, k
        assert peak_err(a[k], b[k]) < 1e-13, (k, peak_err(a[k], b[k]))
    lhs, rhs = (a["y"] * w.numpy()).sum(), (x.numpy() * a["gx"]).sum()
    assert abs(lhs - rhs) <= 1e-13 * abs(lhs)


@pytest.mark.parametrize("o,n", [(147, 160), (160, 147), (441, 160), (640, 147), (2, 1), (1, 2)])
def test_output_length_and_adjoint_of_the_restatement(o, n):
    for N in sorted({1, max(o - 1, 1), o, o + 1, 161}):
        g = torch.Generator().manual_seed(N)
        x = torch.randn(1, N, generator=g, dtype=torch.float64)
        M = -(-n * N // o)
        assert R.forward(x, o, n).shape == (1, M) and R.out_len(o, n, N) == M == math.ceil(n * N / o)
        w = torch.randn(1, M, generator=g, dtype=torch.float64)
        r = R.forward_backward(x, w, o, n)
        lhs, rhs = (r["y"] * w.numpy()).sum(), (x.numpy() * r["gx"]).sum()
        assert abs(lhs - rhs) <= 1e-13 * max(abs(lhs), 1e-3)


# ---- resample_taps -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [HANN, KAISER, R.KAISER_FAST], ids=["hann", "kaiser", "kaiser_fast"])
@pytest.mark.parametrize("o,n,P", [(147, 160, 13), (441, 160, 34), (640, 147, 53), (2, 3, None), (3, 2, None), (1, 2, None)])
def test_taps_against_the_formula_and_the_zero_rule(o, n, P, kw):
    h, width = D.signal.resample_taps(o, n, **kw)
    want, wwidth, inside = R.taps_numpy(o, n, **kw)
    W, rolloff = kw.get("lowpass_filter_width", 6), kw.get("rolloff", 0.99)
    assert width == wwidth == math.ceil(W * o / (min(o, n) * rolloff))
    assert h.dtype == torch.float64 and h.device.type == "cpu" and tuple(h.shape) == (n, 2 * width + o)
    assert np.abs(h.numpy() - want).max() <= 1e-15
    assert not h.numpy()[~inside].any()                                        # exactly zero where t was clamped
    first, cnt = inside.argmax(1), inside.sum(1)
    for r in range(n):                                                         # one compact span per phase: exactly where |t| < W
        assert inside[r, first[r]:first[r] + cnt[r]].all() and cnt[r] == inside[r].sum() >= 1
    if P is not None and kw is HANN:
        assert cnt.max() == P
    assert cnt.max() <= 2 * W * max(1.0, o / n) / rolloff + 2
    t32, twidth, tin = R.design(o, n, **kw)                                    # the restatement's own design: the same taps after rounding
    assert twidth == width and np.array_equal(tin.numpy(), inside)
    assert np.abs(t32.double().numpy() - h.numpy()).max() <= 2.0 ** -24 * np.abs(want).max() + 1e-15


def test_non_reduced_rates_give_the_reduced_design():
    a, wa = D.signal.resample_taps(44100, 48000)
    b, wb = D.signal.resample_taps(147, 160)
    assert wa == wb and torch.equal(a, b)
    assert D.signal.check_resampling(44100, 48000) == (147, 160) and D.signal.check_resampling(48000.0, 16000) == (3, 1)


@pytest.mark.parametrize("o,n", [(147, 160), (160, 147), (441, 160), (80, 441), (640, 147), (2, 1), (1, 2), (3, 2), (2, 3)])
def test_the_two_tables_hold_the_same_filter(o, n):
    """The forward table gives back the float32 taps on their spans; the transposed table, read as the gather it is, equals the scatter
    of the forward one on a short signal, bit for bit in float64 on the float32 taps' products (same products, summed per input)."""
    d = _resample_design.Design(o, n, 6, 0.99, "sinc_interp_hann", None)
    h32 = R.design(o, n)[0].numpy()
    inside = R.design(o, n)[2].numpy()
    f, b = d.fwd, d.bwd
    assert (f.A, f.B, b.A, b.B) == (n, o, o, n) and f.floats == n * f.P and b.floats == o * b.P
    for t in (f, b):
        words = t.words
        assert words.dtype == np.uint32 and words.size == t.A * t.P + t.A
        meta = words[t.A * t.P:]
        assert np.array_equal(meta & 0xffff, t.off - t.lo) and np.array_equal(meta >> 16, t.cnt)
        assert t.span == (t.off + t.cnt).max() - t.lo and t.cnt.max() == t.P and t.span <= 0xffff and t.P < 1 << 15
    T = f.words[:n * f.P].view(np.float32).reshape(f.P, n)
    for r in range(n):
        k0 = f.off[r] + d.width
        assert np.array_equal(T[:f.cnt[r], r], h32[r, k0:k0 + f.cnt[r]]) and not T[f.cnt[r]:, r].any()
        assert np.array_equal(np.nonzero(inside[r])[0], np.arange(k0, k0 + f.cnt[r]))
    N = 3 * o + 5
    M = d.out_len(N)
    g = np.random.default_rng(o * n)
    gy = g.standard_normal(M)
    scatter = np.zeros(N)
    for j in range(M):
        q, r = divmod(j, n)
        for m in range(f.cnt[r]):
            i = q * o + f.off[r] + m
            if 0 <= i < N:
                scatter[i] += float(T[m, r]) * gy[j]
    Tb = b.words[:o * b.P].view(np.float32).reshape(b.P, o)
    gather = np.zeros(N)
    for i in range(N):
        Q, s = divmod(i, o)
        for m in range(b.cnt[s]):
            j = Q * n + b.off[s] + m
            if 0 <= j < M:
                gather[i] += float(Tb[m, s]) * gy[j]
    assert np.abs(gather - scatter).max() <= 1e-15 * np.abs(scatter).max()


# ---- lengths, equal rates, errors --------------------------------------------------------------------------------------------------------
def test_equal_rates_return_the_same_object():
    x = torch.zeros(2, 3, 10)
    assert D.resample(x, 44100, 44100) is x and D.resample(x, 7, 7, resampling_method="sinc_interp_kaiser") is x
    assert D.Resample()(x) is x and D.Resample(48000, 48000)(x) is x


@pytest.mark.parametrize("kw", [dict(orig_freq=44100.5), dict(orig_freq=0), dict(new_freq=-3), dict(new_freq=float("nan")), dict(orig_freq="a"),
                                dict(orig_freq=True), dict(lowpass_filter_width=0), dict(lowpass_filter_width=-2), dict(lowpass_filter_width=2.5),
                                dict(rolloff=0.0), dict(rolloff=1.01), dict(rolloff=float("nan")), dict(resampling_method="linear"),
                                dict(beta=-1.0), dict(beta=float("inf")), dict(beta=float("nan"))])
def test_bad_arguments_raise_value_error(kw):
    a = {**dict(orig_freq=44100, new_freq=48000), **kw}
    for fn in (D.signal.resample_taps, D.signal.check_resampling, lambda **k: D.resample(torch.zeros(1, 8), **k),
               lambda **k: D.Resample(**k)):
        with pytest.raises(ValueError):
            fn(**a)


def test_cpu_tensor_and_float64_are_refused(monkeypatch):
    with pytest.raises(_lib.DaspHipError, match="no CPU path"):
        D.resample(torch.zeros(2, 2, 64), 44100, 48000)
    with pytest.raises(_lib.DaspHipError, match="no CPU path"):
        D.Resample(48000, 16000)(torch.zeros(2, 64))
    monkeypatch.setattr(_lib, "require_device", lambda t, name="x": None)
    with pytest.raises(_lib.DaspHipError, match="resample: float64"):
        D.resample(torch.zeros(2, 64, dtype=torch.float64), 44100, 48000)


def test_too_large_a_design_is_refused_on_the_host(monkeypatch):
    """2049 : 2048 at the defaults: 13 or 14 taps for each of 2048 phases, more than the table holds - NotImplementedError before the
    device is looked at."""
    monkeypatch.setattr(_lib, "require_device", lambda t, name="x": None)
    with pytest.raises(NotImplementedError, match="resample 2049:2048"):
        D.resample(torch.zeros(1, 64), 2049, 2048)


def test_signatures_and_module():
    names = ["orig_freq", "new_freq", "lowpass_filter_width", "rolloff", "resampling_method", "beta"]
    sig = inspect.signature(D.functional.resample)
    assert list(sig.parameters) == ["x"] + names
    assert [sig.parameters[k].default for k in names[2:]] == [6, 0.99, "sinc_interp_hann", None]
    assert list(inspect.signature(D.signal.resample_taps).parameters) == names
    msig = inspect.signature(D.modules.Resample.__init__)
    assert list(msig.parameters)[1:] == ["orig_freq", "new_freq", "resampling_method", "lowpass_filter_width", "rolloff", "beta"]
    assert [p.default for p in list(msig.parameters.values())[1:]] == [16000, 16000, "sinc_interp_hann", 6, 0.99, None]
    m = D.Resample(44100, 48000)
    assert not list(m.parameters()) and not list(m.buffers())
    assert D.resample is D.functional.resample and D.Resample is D.modules.Resample and D.resample_taps is D.signal.resample_taps


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_size_queries():
    L = _lib.lib()
    tmax, wmax = L.dasp_resample_table_limit(), L.dasp_resample_window_limit()
    assert tmax >= 16384 and wmax >= 16384
    for o, n in ((147, 160), (160, 147), (441, 160), (80, 441), (640, 147), (2, 1), (1, 2), (3, 2), (2, 3), (1023, 1024), (1024, 1023), (1024, 1), (1, 1024)):
        d = _resample_design.Design(o, n, 6, 0.99, "sinc_interp_hann", None)
        for t in (d.fwd, d.bwd):
            assert t.floats <= tmax and t.span <= wmax, (o, n)
            T = L.dasp_resample_tile(t.A, t.B, t.P, t.span)
            assert T > 0 and T % t.A == 0, (o, n, T)
            F = T // t.A
            assert F == max(1, min(2048 // t.A, (wmax - t.span) // t.B + 1))
            window = (F - 1) * t.B + t.span
            assert window <= wmax and (t.floats + t.A + window) * 4 <= 158 * 1024
            assert L.dasp_resample_table_words(t.A, t.P) == t.floats + t.A == t.words.size
        if (o, n) == (147, 160):
            assert (d.fwd.P, L.dasp_resample_tile(160, 147, d.fwd.P, d.fwd.span)) == (13, 12 * 160)
    d = _resample_design.Design(147, 160, **R.KAISER_FAST)
    assert d.fwd.floats <= tmax and d.bwd.floats <= tmax and L.dasp_resample_tile(160, 147, d.fwd.P, d.fwd.span) > 0
    assert L.dasp_resample_tile(0, 1, 1, 1) == -1 and L.dasp_resample_tile(1, 0, 1, 1) == -1 and L.dasp_resample_tile(4, 4, 0, 1) == -1
    assert L.dasp_resample_tile(4, 4, 5, 4) == -1                                   # a span shorter than the taps it holds
    assert L.dasp_resample_tile(2048, 2049, 14, 16) == -2 and L.dasp_resample_tile(1, 1, 8, wmax + 1) == -2
    assert L.dasp_resample_tile(tmax, 1, 1, wmax) == -2                             # each inside its limit, together beyond the LDS
    assert L.dasp_resample_table_words(0, 3) == -1 and L.dasp_resample_table_words(3, 0) == -1 and L.dasp_resample_table_words(tmax, 2) == -2


def test_entry_points_check_their_arguments_without_gpu():
    """DASP_ERR_ARG (-1) for null pointers, impossible sizes and inconsistent table arguments, DASP_ERR_UNSUPPORTED (-2) for a design
    beyond the limits and for more than 2^31 - 1 workgroups - all before any launch. The non-null device pointers are fakes, never read."""
    L = _lib.lib()
    f = 256
    ok = dict(rows=4, N=1470, M=1600, o=147, n=160)
    tabs = dict(fwd=dict(P=13, lo=-7, span=14), bwd=dict(P=15, lo=-8, span=16))

    def run(which, a=f, tab=f, b=f, **kw):
        v = {**ok, **tabs[which], **kw}
        fn = L.dasp_resample_forward if which == "fwd" else L.dasp_resample_backward
        return fn(a, tab, b, v["rows"], v["N"], v["M"], v["o"], v["n"], v["P"], v["lo"], v["span"], None)

    for which in ("fwd", "bwd"):
        call = lambda **kw: run(which, **kw)
        assert call(a=None) == -1 and call(tab=None) == -1 and call(b=None) == -1
        assert call(rows=0) == -1 and call(N=0) == -1 and call(M=0) == -1 and call(o=0) == -1 and call(n=-1) == -1
        assert call(M=1599) == -1 and call(M=1601) == -1                     # M is ceil(n N / o)
        assert call(P=0) == -1 and call(P=20, span=19) == -1 and call(lo=-30000) == -1 and call(lo=1000) == -1
        assert call(P=120, span=120) == -2                                   # more than 16384 taps
        assert call(span=30000) == -2
        assert call(rows=1 << 31, N=147 * 10000, M=160 * 10000) == -2         # rows x tiles beyond 2^31 - 1
    assert L.dasp_resample_table_store(None, f, 10, None) == -1 and L.dasp_resample_table_store(f, None, 10, None) == -1
    assert L.dasp_resample_table_store(f, f, 0, None) == -1 and L.dasp_resample_table_store(f, f, 1 << 20, None) == -2


# ---- what the default design rejects: recorded, not bounded -------------------------------------------------------------------------------
def test_alias_rejection_of_the_default_design_is_recorded():
    """48 -> 16 kHz with the default design (Hann, width 6, rolloff 0.99): tones above the new Nyquist frequency of 8 kHz, amplitude 1,
    through the float64 restatement; the figure is the RMS of what comes out over the RMS of a passband tone at 1 kHz (middle half of the
    signal). Recorded for DESIGN 3.15; the only assertion is that the passband is passed."""
    N = 48000
    t = torch.arange(N, dtype=torch.float64) / 48000.0
    rms = lambda y: float(y[len(y) // 4: 3 * len(y) // 4].pow(2).mean().sqrt())
    ref = rms(R.forward(torch.sin(2 * math.pi * 1000.0 * t)[None], 48000, 16000)[0])
    out = {}
    for hz in (8500.0, 9000.0, 10000.0, 12000.0, 15000.0, 20000.0):
        out[hz] = 20 * math.log10(max(rms(R.forward(torch.sin(2 * math.pi * hz * t)[None], 48000, 16000)[0]), 1e-300) / ref)
    record("resample_alias_rejection_48k_to_16k_db", **{f"tone_{int(hz)}": v for hz, v in out.items()}, passband_rms=ref)
    assert abs(ref - math.sqrt(0.5)) < 1e-3


# ---- torchaudio, if it happens to be there -------------------------------------------------------------------------------------------------
def test_restatement_against_torchaudio_if_installed():
    ta = pytest.importorskip("torchaudio")
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 3000, generator=g)
    for o, n, kw in ((44100, 48000, HANN), (48000, 44100, KAISER), (441, 160, HANN)):
        want = ta.functional.resample(x.double(), o, n, **kw).numpy()
        got32, got64 = R.forward(x, o, n, arith=torch.float32, **kw).double().numpy(), R.forward(x, o, n, **kw).numpy()
        e32 = peak_err(got32, got64)
        assert got64.shape == want.shape and peak_err(got64, want) <= max(4 * e32, 2e-6)
