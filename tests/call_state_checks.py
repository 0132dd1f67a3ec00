"""The battery of tests/test_gpu_call_state.py and tests/test_call_state_cpu.py (not collected): seven checks of what a call LEAVES BEHIND
in the process that made it, each a plain function of a `Spec` of tests/autograd_contract_checks.py (S5 and S7: of several). Pure torch:
the CPU file runs S1 - S4 on toy Functions with planted defects.

  S1  every tensor handed in (make(seed), the upstream gradients) keeps its bits and its _version over forward + backward, over the
      no_grad forward, and as a 4-byte-offset view / a row slice of a NaN-filled allocation, whose bytes outside the view stay too
  S2  torch's CPU generator, every device generator, numpy's and random's global generators are where they were - or, for an entry
      documented to draw (spec.draws), the CPU generator is where that one draw leaves it
  S3  current device and stream, default dtype, grad mode, autocast state and every attribute of config.plan are what they were, also
      after a call the library refuses; the next valid call returns the bits of the call before the refusal
  S4  with the garbage collector off, the bytes allocated after every step equal the bytes after warm-up, and a collection afterwards
      finds no unreachable tensor
  S5  a cached constant survives its cache being cleared: 33 streams (or nine keys) cross every limit of 8 and 16
  S6  hipPeekAtLastError() and dasp_device_error() are 0 after the entry
  S7  four host threads, each with its own stream, run the entries of one config.plan side by side

Every check returns a list of findings (strings; empty = nothing left behind) and appends (check, key, measured) to `rec`."""
import contextlib
import gc
import random
import threading

import numpy as np
import torch

from tests import autograd_contract_checks as K

GUARD = 2048                       # elements of NaN before and after a guarded view (tests/input_domain_cases.py)
_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def on_gpu(spec):
    return torch.device(spec.device).type == "cuda"


# ---- bits and versions ------------------------------------------------------------------------------------------------------------------------

def bits(t):
    """The tensor's elements as integers of the same width, on the host (NaN payloads and signed zeros compare as what they are)."""
    v = t.detach()
    if v.is_complex():
        v = torch.view_as_real(v.resolve_conj())
    v = v.clone(memory_format=torch.contiguous_format)
    if v.dtype is torch.bool:
        v = v.to(torch.uint8)
    return v.view(_INT[v.element_size()]).cpu()


def snapshot(tensors):
    return {n: (bits(v), v._version) for n, v in tensors.items() if isinstance(v, torch.Tensor)}


def changed(before, tensors, what):
    find = []
    for n, (b0, v0) in before.items():
        v = tensors[n]
        if not torch.equal(bits(v), b0):
            find.append(f"S1 {what} {n}: its bits changed")
        if v._version != v0:
            find.append(f"S1 {what} {n}: _version {v0} -> {v._version}")
    return find


@contextlib.contextmanager
def isolated():
    """What a check needs of the process to go on after an op that left something behind: grad mode and default dtype put back."""
    grad, dt = torch.is_grad_enabled(), torch.get_default_dtype()
    try:
        yield
    finally:
        torch.set_grad_enabled(grad)
        torch.set_default_dtype(dt)


def step(spec, seed, gys=None, change=None, no_grad=False, watch=None):
    """One forward (+ one backward over all leaves) like checks.run; watch: a list that receives the S1 findings of this step - the bits
    and versions of every tensor handed in, and of watch-ed base allocations, before against after."""
    with isolated():
        t = K.leafed(spec, seed, () if no_grad else spec.leaves, change)
        bases = getattr(change, "bases", {}) if change is not None else {}
        before = snapshot(t) if watch is not None else None
        before_b = snapshot(bases) if watch is not None else None
        with (torch.no_grad() if no_grad else contextlib.nullcontext()):
            outs = K.outputs(spec, t)
        res = {"y%d" % i: o.detach() for i, o in enumerate(outs)}
        if spec.leaves and not no_grad:
            gys = K.upstream(outs, 0) if gys is None else gys
            g = {"gy%d" % i: v for i, v in enumerate(gys)}
            before_g = snapshot(g) if watch is not None else None
            torch.autograd.backward(outs, gys)
            res["_gys"] = gys
        for n in spec.leaves:
            res["g_" + n] = t[n].grad
        K.sync(spec)
        if watch is not None:
            tag = getattr(change, "tag", "no_grad" if no_grad else "as_is")
            watch += changed(before, t, tag) + changed(before_b, bases, tag + " base allocation of")
            if spec.leaves and not no_grad:
                watch += changed(before_g, g, tag)
        return res


# ---- S1: arguments keep their bits and versions ------------------------------------------------------------------------------------------------

def _movable(v):
    return isinstance(v, torch.Tensor) and (v.is_floating_point() or v.is_complex()) and v.numel() > 0 and v.dim() > 0


def offset_views():
    """change(t): every floating tensor as a contiguous view one element (4 bytes of float32) past a 16-byte boundary of a NaN-filled
    allocation, GUARD elements of NaN on either side."""
    def change(t):
        for n, v in list(t.items()):
            if _movable(v):
                buf = torch.full((2 * GUARD + v.numel() + 8,), float("nan"), dtype=v.dtype, device=v.device)
                view = buf[GUARD + 1:GUARD + 1 + v.numel()].view(v.shape)
                view.copy_(v)
                t[n] = view
                change.bases[n] = buf
    change.bases, change.tag = {}, "offset_views"
    return change


def row_slices(names):
    """change(t): the named tensors as the slice wide[..., 9:9 + N] of a wider NaN tensor - not contiguous."""
    def change(t):
        for n in names:
            v = t[n]
            if _movable(v):
                wide = torch.full(v.shape[:-1] + (v.shape[-1] + 21,), float("nan"), dtype=v.dtype, device=v.device)
                view = wide[..., 9:9 + v.shape[-1]]
                view.copy_(v)
                t[n] = view
                change.bases[n] = wide
    change.bases, change.tag = {}, "row_slices"
    return change


def check_arguments(spec, rec, seed=0):
    find = []
    base = step(spec, seed, watch=find)
    gys = base.get("_gys")
    step(spec, seed, no_grad=True, watch=find)
    ys = K.y_keys(base)
    for change in (offset_views(), row_slices(spec.audio if spec.audio else tuple(spec.forms))):
        moved = None
        if gys is not None:                     # the upstream gradients in the same layout, their allocations watched with the rest
            moved = {"gy%d" % i: g for i, g in enumerate(gys)}
            mover = offset_views() if change.tag == "offset_views" else row_slices(tuple(moved))
            mover(moved)
            change.bases.update({"upstream " + n: b for n, b in mover.bases.items()})
        got = step(spec, seed, gys=gys if moved is None else [moved["gy%d" % i] for i in range(len(gys))], change=change, watch=find)
        if not change.bases or getattr(spec, "draws", None) is not None:      # (an entry that draws has other noise in every call)
            continue
        # (the same numbers through other pointers: the values are the off-domain tests' business, here they only have to be there)
        for k in ys + K.grad_keys(spec):
            rec.append(("S1." + change.tag, k, K.rel(got.get(k), base.get(k)) if got.get(k) is not None else 0.0))
    rec.append(("S1.findings", "count", float(len(find))))
    return find


# ---- S2: random-number state --------------------------------------------------------------------------------------------------------------------

def rng_states(spec):
    np_state = np.random.get_state()
    return {"torch CPU generator": torch.get_rng_state(),
            "device generators": [s.clone() for s in torch.cuda.get_rng_state_all()] if on_gpu(spec) else [],
            "numpy.random": (np_state[0], np_state[1].copy()) + tuple(np_state[2:]),
            "random": random.getstate()}


def _equal(a, b):
    if isinstance(a, torch.Tensor):
        return torch.equal(a, b)
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_equal(x, y) for x, y in zip(a, b))
    return a == b


def check_rng(spec, rec, seed=0):
    find = []
    draws = getattr(spec, "draws", None)
    for what, no_grad in (("forward + backward", False), ("no_grad forward", True)):
        # the check's own draws first: a generator that was only just seeded would hide an op that seeds it again with the same number
        torch.rand(3)
        if on_gpu(spec):
            torch.rand(3, device=spec.device)
        s0 = rng_states(spec)
        step(spec, seed, no_grad=no_grad)
        s1 = rng_states(spec)
        want = s0["torch CPU generator"]
        if draws is not None:
            torch.set_rng_state(s0["torch CPU generator"])
            draws()
            want = torch.get_rng_state()          # (and the generator stays there: where the entry's call leaves it)
        for k in s0:
            ok = _equal(s1[k], want if k == "torch CPU generator" else s0[k])
            rec.append(("S2." + what.split()[0], k, 0.0 if ok else 1.0))
            if not ok:
                find.append(f"S2 {what}: {k} " + ("is not where the documented draw leaves it" if k == "torch CPU generator" and draws else "changed"))
    return find


# ---- S3: ambient settings -----------------------------------------------------------------------------------------------------------------------

def ambient(spec):
    out = {"default dtype": torch.get_default_dtype(), "grad mode": torch.is_grad_enabled(),
           "autocast": tuple((torch.is_autocast_enabled(d), torch.get_autocast_dtype(d)) for d in ("cuda", "cpu"))}
    if on_gpu(spec):
        from dasp_pytorch_amd import config
        out["current device"] = torch.cuda.current_device()
        out["current stream"] = int(torch.cuda.current_stream().cuda_stream)
        for k in sorted(n for n in dir(type(config.plan)) if not n.startswith("_")):
            out["config.plan." + k] = getattr(config.plan, k)
    return out


def check_ambient(spec, rec, seed=0, refusal=None):
    """refusal: (what, change(t) or None, call(t) or None) - a call the library refuses on the host."""
    find = []
    a0 = ambient(spec)
    with isolated():
        t = K.leafed(spec, seed, spec.leaves)
        outs = K.outputs(spec, t)
        a1 = ambient(spec)
        if spec.leaves:
            torch.autograd.backward(outs, K.upstream(outs, 0))
        K.sync(spec)
        a2 = ambient(spec)
    for when, a in (("after the forward", a1), ("after the backward", a2)):
        for k in a0:
            rec.append(("S3." + when.split()[-1], k, 0.0 if a[k] == a0[k] else 1.0))
            if a[k] != a0[k]:
                find.append(f"S3 {when}: {k} {a0[k]!r} -> {a[k]!r}")
    if refusal is not None:
        what, change, call = refusal
        before = step(spec, seed)
        raised = None
        with isolated():
            t = K.leafed(spec, seed, spec.leaves, change)
            try:
                (call or spec.call)(t)
            except Exception as e:             # noqa: BLE001 - any refusal, by whatever exception the op documents
                raised = e
            ar = ambient(spec)
        K.sync(spec)
        rec.append(("S3.refused", "raised", 1.0 if raised is not None else 0.0))
        if raised is None:
            find.append(f"S3 {what}: not refused")
        for k in a0:
            if ar[k] != a0[k]:
                find.append(f"S3 after the refusal of {what}: {k} {a0[k]!r} -> {ar[k]!r}")
        if on_gpu(spec):
            from dasp_pytorch_amd import _lib
            err = int(_lib.lib().dasp_device_error())
            rec.append(("S3.refused", "dasp_device_error", float(err)))
            if err:
                find.append(f"S3 after the refusal of {what}: dasp_device_error() = {err:#x}")
        after = step(spec, seed, gys=before.get("_gys"))
        find += K.same(spec, "S3.after_refusal_vs_before", K.y_keys(before) + K.grad_keys(spec), after, before, rec, f"[{what}]")
    return find


# ---- S4: memory ---------------------------------------------------------------------------------------------------------------------------------

def live_tensor_bytes():
    """A byte counter without a device: the elements of every tensor object alive."""
    import warnings
    with warnings.catch_warnings():              # (isinstance on every object alive wakes a few deprecated module attributes)
        warnings.simplefilter("ignore")
        return sum(o.numel() * o.element_size() for o in gc.get_objects() if isinstance(o, torch.Tensor))


def check_memory(spec, rec, seed=0, counter=None, steps=5):
    cuda = on_gpu(spec) and counter is None
    counter = counter or torch.cuda.memory_allocated
    find = []
    was = gc.isenabled()
    gc.collect()
    gc.disable()
    try:
        start = counter()
        gys = step(spec, seed).get("_gys")              # warm-up 1 (it also makes the upstream gradients, which stay)
        step(spec, seed, gys=gys)                       # warm-up 2
        warm = counter()
        if cuda:
            torch.cuda.reset_peak_memory_stats()
        for i in range(steps):
            step(spec, seed, gys=gys)
            now = counter()
            rec.append(("S4.bytes_over_warm", "step%d" % i, float(now - warm)))
            if now != warm:
                find.append(f"S4 step {i + 1} after warm-up: {now} bytes allocated, {warm} after warm-up ({now - warm:+d})")
        peak = torch.cuda.max_memory_allocated() - warm if cuda else 0
        block = 512 if cuda else 1                      # (the caching allocator hands out multiples of 512 bytes)
        gy_bytes = sum(-(-g.numel() * g.element_size() // block) * block for g in gys) if gys else 0
        rec.append(("S4.bytes_held", "caches_after_warm_up", float(warm - start - gy_bytes)))
        rec.append(("S4.bytes_peak", "above_warm", float(peak)))
        gc.set_debug(gc.DEBUG_SAVEALL)
        try:
            gc.collect()
            lost = [o for o in gc.garbage if isinstance(o, torch.Tensor)]
        finally:
            gc.set_debug(0)
            gc.garbage.clear()
        rec.append(("S4.unreachable", "tensors", float(len(lost))))
        if lost:
            find.append(f"S4 {len(lost)} tensors were unreachable but alive until a garbage collection: " +
                        ", ".join(sorted({f"{tuple(o.shape)} {o.dtype}" for o in lost})[:6]))
        del lost
    finally:
        if was:
            gc.enable()
        gc.collect()
    return find


# ---- S6: error state ----------------------------------------------------------------------------------------------------------------------------

_hip = []


def hip_runtime():
    """The libamdhip64 the process has loaded already (its path read from the process's own map), through ctypes."""
    if not _hip:
        import ctypes
        path = None
        with open("/proc/self/maps") as f:
            for line in f:
                if "libamdhip64" in line:
                    path = line.split()[-1]
                    break
        assert path, "no libamdhip64 is loaded in this process"
        lib = ctypes.CDLL(path)
        for fn in (lib.hipPeekAtLastError, lib.hipGetLastError):
            fn.restype, fn.argtypes = ctypes.c_int, []
        _hip.append(lib)
    return _hip[0]


def error_words(rec, what):
    from dasp_pytorch_amd import _lib
    torch.cuda.synchronize()
    hip, dasp = int(hip_runtime().hipPeekAtLastError()), int(_lib.lib().dasp_device_error())
    rec.append(("S6." + what, "hipPeekAtLastError", float(hip)))
    rec.append(("S6." + what, "dasp_device_error", float(dasp)))
    return ([f"S6 {what}: hipPeekAtLastError() = {hip}"] if hip else []) + ([f"S6 {what}: dasp_device_error() = {dasp:#x}"] if dasp else [])


def check_errors(spec, rec, seed=0):
    """(What an earlier test left in the runtime's error word is read out first - that resets it - and recorded, not judged.)"""
    torch.cuda.synchronize()
    rec.append(("S6.before", "hipGetLastError", float(hip_runtime().hipGetLastError())))
    step(spec, seed)
    find = error_words(rec, "after_forward_backward")
    step(spec, seed, no_grad=True)
    return find + error_words(rec, "after_no_grad_forward")


CHECKS = {"S1_arguments": check_arguments, "S2_rng": check_rng, "S3_ambient": check_ambient, "S4_memory": check_memory, "S6_errors": check_errors}


# ---- references of a run ------------------------------------------------------------------------------------------------------------------------

def reference_of(spec, seed, gys, state=None):
    if getattr(spec, "reference_at", None) is not None:
        return spec.reference_at(state, seed, gys)
    return spec.reference(seed, gys) if spec.reference else None


def held(spec, check, got, want_run, ref, rec, what):
    """got against another run by the `same` rule and against the float64 reference at the entry's existing bound."""
    keys = K.y_keys(want_run) + K.grad_keys(spec)
    find = K.same(spec, check + ".vs_first_run", keys, got, want_run, rec, what)
    if ref is not None and spec.compare:
        find += spec.compare(keys, got, ref, rec, check + ".vs_float64" + what)
    return find


# ---- S5: cache eviction -------------------------------------------------------------------------------------------------------------------------

def cache_sizes(caches, rec, find, what):
    import importlib
    for module, attr, limit in caches:
        n = len(getattr(importlib.import_module(module), attr))
        rec.append(("S5.cache_size", attr, float(n)))
        if n > limit:
            find.append(f"S5 {what}: {attr} holds {n} entries, its limit is {limit}")


def check_eviction(specs, caches, mode, rec, seed=0, streams=32):
    """mode "streams": the one entry on the default stream, on `streams` new ones, and on the default stream again; mode "entries": every
    entry (one cache key each) on the default stream, then the first again."""
    find = []
    held0 = torch.cuda.memory_allocated()
    if mode == "streams":
        spec = specs[0]
        runs = [(spec, None)] + [(spec, torch.cuda.Stream(device=spec.device)) for _ in range(streams)] + [(spec, None)]
    else:
        runs = [(s, None) for s in specs] + [(specs[0], None)]
    first = {}
    for i, (spec, stream) in enumerate(runs):
        state = torch.get_rng_state()
        with (torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()):
            got = step(spec, seed, gys=first[spec.name][0].get("_gys") if spec.name in first else None)
        torch.cuda.synchronize()
        if spec.name not in first:
            first[spec.name] = (got, reference_of(spec, seed, got.get("_gys") or [], state))
        base, ref = first[spec.name]
        find += held(spec, "S5", got, base, ref, rec, f"[run {i}]")
        cache_sizes(caches, rec, find, f"run {i}")
        proc = getattr(spec, "proc", None)
        if proc is not None:
            n = len(proc.__dict__.get("_affine_cache", {}))
            rec.append(("S5.cache_size", "_affine_cache", float(n)))
            if n > 8:
                find.append(f"S5 run {i}: _affine_cache holds {n} entries, its limit is 8")
    first.clear()
    got = base = ref = None
    rec.append(("S5.bytes_held", "after_the_last_run", float(torch.cuda.memory_allocated() - held0)))
    return find


# ---- S7: host threads ---------------------------------------------------------------------------------------------------------------------------

GLOBAL_GENERATOR = threading.Lock()     # an entry whose call seeds and draws from the process-global CPU generator takes it for its forward


def check_threads(specs, rec, seed=0, threads=4, rounds=3):
    """The entries (all of one config.plan) serially, then `threads` host threads, each with a stream of its own, starting from a barrier:
    in round r thread i runs the entries [(i + r) % threads :: threads], forward + backward. Every result is held to the serial run and
    to the float64 reference; S1 holds per thread. An entry with spec.global_generator makes its forward under one lock: it seeds the
    process-global CPU generator and draws from it, which two threads cannot do side by side in any library."""
    find = []
    serial, refs = {}, {}
    for spec in specs:
        state = torch.get_rng_state()
        serial[spec.name] = step(spec, seed)
        refs[spec.name] = reference_of(spec, seed, serial[spec.name].get("_gys") or [], state)
        find += held(spec, "S7.serial", serial[spec.name], serial[spec.name], refs[spec.name], rec, "")
    torch.cuda.synchronize()
    barrier = threading.Barrier(threads)
    results, errors = [[] for _ in range(threads)], []

    def work(i):
        try:
            stream = torch.cuda.Stream(device=specs[0].device)
            barrier.wait(timeout=60)
            with torch.cuda.stream(stream):
                for r in range(rounds):
                    for spec in specs[(i + r) % threads::threads]:
                        s1 = []
                        with (GLOBAL_GENERATOR if getattr(spec, "global_generator", False) else contextlib.nullcontext()):
                            # (step() makes forward and backward; the lock is held over both, which costs this entry its overlap only)
                            got = step(spec, seed, gys=serial[spec.name].get("_gys"), watch=s1)
                        results[i].append((spec, r, got, s1))
        except BaseException as e:              # noqa: BLE001 - reported by the caller, in the main thread
            errors.append((i, e))
            try:
                barrier.abort()
            except Exception:                    # noqa: BLE001
                pass
    pool = [threading.Thread(target=work, args=(i,), name=f"S7-{i}", daemon=True) for i in range(threads)]
    for th in pool:
        th.start()
    for th in pool:
        th.join(timeout=120)
    stuck = [th.name for th in pool if th.is_alive()]
    if stuck:
        return find + [f"S7 threads {stuck} did not finish within 120 s"]
    torch.cuda.synchronize()
    for i, e in errors:
        if not isinstance(e, threading.BrokenBarrierError):
            raise e
    for i, res in enumerate(results):
        for spec, r, got, s1 in res:
            find += [f"thread {i} round {r} {spec.name}: {m}" for m in s1]
            find += [f"thread {i} round {r} {spec.name}: {m}" for m in held(spec, "S7", got, serial[spec.name], refs[spec.name], rec, "")]
    rec.append(("S7.runs", "count", float(sum(len(r) for r in results))))
    return find
