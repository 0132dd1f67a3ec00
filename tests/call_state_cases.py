"""What tests/test_gpu_call_state.py and tests/test_call_state_cpu.py run beside the table of tests/autograd_contract_cases.py (not
collected): the entries that table cannot hold because they draw from the global CPU generator by design, are not differentiable, or
keep state between calls; the refused calls of S3; the cache families of S5; and the entries a check leaves out, by name and with the
reason. The checks are in tests/call_state_checks.py.

An added entry is a checks.Spec with two more attributes:
  draws              () -> None: the ONE draw from the global CPU generator the entry is documented to make (None: it makes none)
  reference_at       (state, seed, gys) -> {key: float64 array}: the float64 reference of a call made while the CPU generator held
                     `state` (drawn from a private generator set to that state: the global one is not touched), or None"""
import functools

import numpy as np
import torch

from tests import autograd_contract_cases as T
from tests import input_domain_cases as idc
from tests.autograd_contract_checks import Spec

DEV, SR = T.DEV, T.SR
L, TAPS = 256, 31
ROW = L + TAPS - 1


def private(state):
    g = torch.Generator()
    g.set_state(state)
    return g


def _reverb_arrays(seed, B=2, C=2, N=100):
    g = T.gen(seed, 5, B)
    return dict(x=torch.rand(B, C, N, generator=g) * 2 - 1, gains=torch.rand(B, 12, generator=g), decays=torch.rand(B, 12, generator=g),
                mix=torch.rand(B, generator=g))


def _reverb_ref(a, noise, gys):
    n = {k: v.numpy() for k, v in a.items()}
    p = [n[k].astype(np.float64) for k in ("gains", "decays", "mix")]
    y = idc.orc.noise_shaped_reverberation(n["x"], SR, *p, noise, L, TAPS)
    gx, gg, gd, gm = idc.orc.noise_shaped_reverberation_vjp(n["x"], SR, *p, noise, T.as_np(gys[0]), L, TAPS)
    return dict(y0=y, g_x=gx, g_gains=gg, g_decays=gd, g_mix=gm)


REV_TOL = dict(y0=("peak", 2e-5), g_x=("peak", 2e-5), g_gains=("peak", 1e-4), g_decays=("peak", 1e-4), g_mix=("max", 1e-4))   # tests/test_gpu_reverb.py:60-62
REV_SAME = {"y0": 2e-6, "g_x": 2e-6, "g_gains": 1e-5, "g_decays": 1e-5, "g_mix": 1e-5}                                          # tests/test_gpu_reverb.py:184-185
REV_LEAVES = ("x", "gains", "decays", "mix")


def _entry(name, arrays, call, leaves, audio, plan=None, same=None, tol=None, draws=None, reference_at=None, on_device=False, outs=None, cite=""):
    cached = functools.lru_cache(maxsize=4)(arrays)

    def make(seed, device=None):
        return {k: v.to(device or DEV).clone() for k, v in cached(seed).items()}
    spec = Spec(name, make, call, leaves, audio=audio, device=DEV, same=same, compare=T.comparer(T.lists(tol)) if tol else None, plan=plan,
                on_device=on_device, outs=outs, cite=cite)
    spec.draws = draws
    spec.reference_at = (lambda state, seed, gys: reference_at(cached(seed), state, gys)) if reference_at else None
    return spec


@functools.lru_cache(maxsize=1)
def extras():
    E = []
    rev_out = lambda seed: [((2, 2, 100), False)]
    for b in ("ctypes", "torch_ops"):
        plan = {"torch_ops": b == "torch_ops"}

        def call_default(t, **kw):
            cols = [t[k][:, i] for k in ("gains", "decays") for i in range(12)]
            return T.D().noise_shaped_reverberation(t["x"], SR, *cols, t["mix"], num_samples=L, num_bandpass_taps=TAPS, **kw)

        def ref_default(a, state, gys):
            return _reverb_ref(a, torch.randn(4, 12, ROW, generator=private(state)).numpy(), gys)
        E.append(_entry(f"reverb_default_noise[{b}]", _reverb_arrays, call_default, REV_LEAVES, ("x",), plan, REV_SAME, REV_TOL,
                        draws=lambda: torch.randn(4, 12, ROW), reference_at=ref_default, outs=rev_out, cite="tests/test_gpu_reverb.py:60-62, 184-185"))

        def ref_unseeded(a, state, gys):
            """noise_seed=None: one 63-bit draw is the seed; the stream of that seed as dasp_reverb_noise writes it out (needs the device)."""
            from dasp_pytorch_amd import ops
            seed = int(torch.empty((), dtype=torch.int64).random_(generator=private(state)).item())
            return _reverb_ref(a, ops.reverb_noise(seed, 2, 12, ROW, DEV).cpu().numpy(), gys)
        E.append(_entry(f"reverb_device_noise_unseeded[{b}]", _reverb_arrays, functools.partial(call_default, device_noise=True, noise_seed=None),
                        REV_LEAVES, ("x",), plan, REV_SAME, REV_TOL, draws=lambda: torch.empty((), dtype=torch.int64).random_(),
                        reference_at=ref_unseeded, on_device=True, outs=rev_out, cite="tests/test_gpu_reverb.py:60-62, 231, 247"))
    for n in (17, 2 * 159744 + 123):
        def call_stream(t, n=n):
            from dasp_pytorch_amd import _mt19937
            return _mt19937.randn_cpu_stream(n, device=DEV)
        E.append(_entry(f"randn_cpu_stream_n{n}", lambda seed: {}, call_stream, (), (), tol=dict(y0=("max", 1e-6)),       # tests/test_gpu_mtrand.py:48
                        draws=lambda n=n: torch.randn(n), reference_at=lambda a, state, gys, n=n: dict(y0=torch.randn(n, generator=private(state)).numpy()),
                        outs=lambda seed, n=n: [((n,), False)], cite="tests/test_gpu_mtrand.py:48"))

    def call_noise(t):
        from dasp_pytorch_amd import _ctypes_ops
        return _ctypes_ops.reverb_noise(77, 2, 12, ROW, DEV)
    E.append(_entry("reverb_noise_stream", lambda seed: {}, call_noise, (), (), on_device=True, outs=lambda seed: [((4, 12, ROW), False)],
                    cite="the counter-based stream itself: its values are tests/test_gpu_reverb.py:231-260's"))
    for mode in (True, "deferred"):
        def arrays(seed):
            g = T.gen(seed, 17)
            p = lambda n: torch.rand(3, n, generator=g) * 0.9 + 0.05
            return dict(x=torch.rand(3, 2, 1028, generator=g) * 2 - 1, eq=p(18), comp=p(6), rev=p(25), gain=p(1))

        def call_chain(t, mode=mode):
            chain = _chain(mode)
            y = chain.process_normalized(t["x"], t["eq"], t["comp"], t["rev"], t["gain"])
            chain.flush_range_check()
            return y
        E.append(_entry(f"style_transfer_chain[{mode}]", arrays, call_chain, ("x", "eq", "comp", "rev", "gain"), ("x",),
                        same=dict({"y0": 2e-6, "g_x": 2e-6}, **{"g_" + k: 1e-4 for k in ("eq", "comp", "rev", "gain")}), tol=CHAIN_TOL,
                        draws=lambda: torch.randn(6, 12, ROW), reference_at=_chain_ref, outs=lambda seed: [((3, 2, 1028), False)],
                        cite="__graft_entry__.smoke (the chain against the reference's float64 run), tests/test_gpu_chain.py:111"))
    names = [e.name for e in E]
    assert len(set(names)) == len(names)
    return E


# the whole chain's bounds are smoke()'s (y but at the EQ -> compressor stage's 2e-5 of tests/test_gpu_chain.py:111; grad x 2e-5; every
# parameter gradient 1e-4 of its tensor's largest entry)
CHAIN_TOL = dict(y0=("peak", 2e-5), g_x=("peak", 2e-5), g_eq=("max", 1e-4), g_comp=("max", 1e-4), g_rev=("max", 1e-4), g_gain=("max", 1e-4))


def _chain_ref(a, state, gys):
    """EQ -> compressor (the chain's gain added to its make-up gain) -> reverb on the noise torch.randn(2 bs, 12, L + taps - 1) hands out
    from `state`, in float64 from the stages' exact references; the gradients stage by stage backwards, times the parameter spans."""
    chain = _chain(True)
    ranges = lambda proc: np.array([[float(r[0]), float(r[1]) - float(r[0])] for r in proc.param_ranges.values()])
    eq, comp, rev, gain = (ranges(p) for p in (chain.equalizer, chain.compressor, chain.reverb, chain.gain))
    n = {k: v.double().numpy() for k, v in a.items()}
    x = a["x"].numpy()
    p = eq[:, 0] + n["eq"] * eq[:, 1]
    c = comp[:, 0] + n["comp"] * comp[:, 1]
    c[:, 5] += gain[0, 0] + n["gain"][:, 0] * gain[0, 1]
    r = rev[:, 0] + n["rev"] * rev[:, 1]
    noise = torch.randn(6, 12, ROW, generator=private(state)).numpy()
    y1 = idc.peq_exact(x, SR, p)
    y2 = idc.compressor_ref(y1, SR, c, None)
    y = idc.orc.noise_shaped_reverberation(y2, SR, r[:, :12], r[:, 12:24], r[:, 24], noise, L, TAPS)
    g2, gg, gd, gm = idc.orc.noise_shaped_reverberation_vjp(y2, SR, r[:, :12], r[:, 12:24], r[:, 24], noise, T.as_np(gys[0]), L, TAPS)
    _, g1, gc = idc.compressor_ref(y1, SR, c, g2)
    _, gx, gp = idc.peq_exact(x, SR, p, g1)
    return dict(y0=y, g_x=gx, g_eq=gp * eq[:, 1], g_comp=gc * comp[:, 1], g_rev=np.concatenate([gg, gd, gm[:, None]], 1) * rev[:, 1],
                g_gain=(gc[:, 5] * gain[0, 1])[:, None])


@functools.lru_cache(maxsize=2)
def _chain(mode):
    from dasp_pytorch_amd.chain import StyleTransferChain
    chain = StyleTransferChain(SR, num_samples=L, num_bandpass_taps=TAPS)
    for p in (chain.equalizer, chain.compressor, chain.reverb, chain.gain):
        p.validate_range = mode
    return chain


def entries():
    return list(T.table()) + list(extras())


def by_name():
    return {e.name: e for e in entries()}


# ---- entries a check leaves out: by name, with the reason (at most 5 of the table's 112 per check) --------------------------------------------

_SEEDS = "the entry's own call() begins with torch.manual_seed(4242), which reseeds the CPU and every device generator: the test's doing, " \
         "not the library's - reverb_default_noise[...] is the same call without it"
EXEMPT = {
    "S2_rng": {f"reverb_cpu_generator{m}[{b}]": _SEEDS for m in ("", "_mono") for b in ("ctypes", "torch_ops")},
}


# ---- S3: one refused call per family ------------------------------------------------------------------------------------------------------
# Every one is refused on the host before any launch (the line that refuses it is cited). name of the entry -> (what, change(t) or a call).

def _shorter(name):
    def change(t):
        t[name] = t[name][:-1].contiguous()
    return change


def _on_cpu(name):
    def change(t):
        t[name] = t[name].cpu()
    return change


def _double(name):
    def change(t):
        t[name] = t[name].double()
    return change


def _even_taps(t):
    cols = [t["params.%02d" % i] for i in range(25)]
    return T.D().noise_shaped_reverberation(t["x"], SR, *cols, num_samples=L, num_bandpass_taps=TAPS - 1, noise=t["noise"])


REFUSALS = {
    # a control with the wrong batch size
    "gain[ctypes]": ("gain_db with 2 values for 3 items (functional.py: gain)", _shorter("gain_db"), None),
    "gain[torch_ops]": ("gain_db with 2 values for 3 items (functional.py: gain)", _shorter("gain_db"), None),
    "compressor[ctypes]": ("a control with 2 values for 3 items (functional.py: _dynamics)", _shorter("params.02"), None),
    "compressor[torch_ops]": ("a control with 2 values for 3 items (functional.py: _dynamics)", _shorter("params.02"), None),
    "parametric_eq[ctypes]": ("a control with 2 values for 3 items (functional.py: parametric_eq)", _shorter("params.04"), None),
    "parametric_eq[torch_ops]": ("a control with 2 values for 3 items (functional.py: parametric_eq)", _shorter("params.04"), None),
    "stereo_mix": ("pan with 2 rows for 3 items (functional.py: stereo_mix)", _shorter("pan"), None),
    "modulated_delay": ("mix with 2 values for 3 items (functional.py: modulated_delay)", _shorter("mix"), None),
    # float64 into an op without a double path
    "stereo_widener": ("float64 x (ops64.require_fp32_ok)", _double("x"), None),
    "stereo_bus": ("float64 x (ops64.require_fp32_ok)", _double("x"), None),
    "peak_normalize": ("float64 x (functional._level_rows)", _double("x"), None),
    # a tensor on the CPU
    "oversampled_distortion_x4": ("x on the CPU (_lib.require_device)", _on_cpu("x"), None),
    "loudness_one_segment": ("x on the CPU (_lib.require_device)", _on_cpu("x"), None),
    "mrstft_linear": ("target on the CPU (losses._pair_rows; tests/test_gpu_modules.py:322)", _on_cpu("target"), None),
    # odd / even taps
    "reverb_noise[ctypes]": ("an even num_bandpass_taps (functional.py: noise_shaped_reverberation)", None, _even_taps),
    "reverb_noise[torch_ops]": ("an even num_bandpass_taps (functional.py: noise_shaped_reverberation)", None, _even_taps),
}


# ---- S5: cached-constant families -----------------------------------------------------------------------------------------------------------
# name -> (entry or list of entries, [(module, attribute, limit)] of the Python caches it fills, "streams" | "entries")

def taps_entries():
    """The explicit-noise reverb at nine different num_bandpass_taps: nine keys of functional._FB_CACHE (limit 8)."""
    out = []
    for taps in range(15, 32, 2):
        out.append(T.from_idc("reverb_noise", (2, 2, 100), ("ReverbFunction", "_StackColumns"), "ctypes", kw=dict(L=L, taps=taps), same=T.REV_SAME,
                              name=f"reverb_noise_taps{taps}"))
    return out


def affine_entries():
    """modules.Gain at nine parameter ranges: nine keys of the processor's _affine_cache (limit 8). Reference: x 10^((lo + p (hi - lo)) / 20)
    in float64, at gain's own bounds (tests/test_gpu_elementwise.py:83-84, 89)."""
    from dasp_pytorch_amd import modules
    proc = modules.Gain(SR)
    out = []
    for k in range(9):
        lo, hi = -24.0 + k, 24.0 - k

        def arrays(seed):
            g = T.gen(seed, 23)
            return dict(x=torch.rand(3, 2, 1028, generator=g) * 2 - 1, p=torch.rand(3, 1, generator=g) * 0.9 + 0.05)

        def call(t, lo=lo, hi=hi):
            proc.param_ranges = {"gain_db": (lo, hi)}
            return proc.process_normalized(t["x"], t["p"])

        def ref(a, gys, lo=lo, hi=hi):
            x, p = a["x"].double().requires_grad_(True), a["p"].double().requires_grad_(True)
            y = x * (10.0 ** ((lo + p * (hi - lo)) / 20.0)).view(-1, 1, 1)
            y.backward(torch.from_numpy(gys[0]))
            return dict(y0=y.detach().numpy(), g_x=x.grad.numpy(), g_p=p.grad.numpy())
        e = T.simple(f"gain_module_range{k}", arrays, call, ("x", "p"), ("x",), (), dict(y0=("abs1", 2e-6), g_x=("abs1", 2e-6), g_p=("max", 1e-4)), ref,
                     plan={"torch_ops": True}, cite="tests/test_gpu_elementwise.py:83-84, 89")
        e.proc = proc
        out.append(e)
    return out


def families():
    by = by_name()
    return {
        "counters[ctypes]": ([by["compressor_seg[ctypes]"]], [("dasp_pytorch_amd._ctypes_ops", "_DYN_COUNTERS", 16)], "streams"),
        "counters[torch_ops]": ([by["compressor_seg[torch_ops]"]], [], "streams"),
        "mrstft_linear": ([by["mrstft_linear"]], [("dasp_pytorch_amd.losses", "_TW", 16)], "streams"),
        "mrstft_mel": ([by["mrstft_mel"]], [("dasp_pytorch_amd.losses", "_TW", 16), ("dasp_pytorch_amd.losses", "_MEL_DEV", 64)], "streams"),
        "mrstft_aw": ([by["mrstft_aw"]], [("dasp_pytorch_amd.losses", "_TW", 16), ("dasp_pytorch_amd.losses", "_FIR_DEV", 16)], "streams"),
        "filter_spectrum": ([by["reverb_cpu_generator[ctypes]"]], [("dasp_pytorch_amd._ctypes_ops", "_FSPEC_CACHE", 8)], "streams"),
        "filterbank": (taps_entries(), [("dasp_pytorch_amd.functional", "_FB_CACHE", 8), ("dasp_pytorch_amd._ctypes_ops", "_FSPEC_CACHE", 8)], "entries"),
        "fdfir_twiddles": ([by["freqdomain_fir_n64"]], [], "streams"),
        "affine": (affine_entries(), [], "entries"),
    }
