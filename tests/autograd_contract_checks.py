"""The battery of tests/test_gpu_autograd_contract.py and tests/test_autograd_contract_cpu.py (not collected): seven checks of what a
torch.autograd.Function owes autograd, each a plain function of a `Spec` - a callable that builds a fresh graph, with the little the
checks need to know about it. Pure torch: the CPU file runs the same functions on toy Functions with planted defects.

A Spec has
  name, device
  make(seed)   -> {name: tensor on `device`}: fresh tensors, none requiring a gradient, the same values for the same seed
  call(t)      -> tuple of output tensors, from the tensors t[name] (a leaf is t[name] itself: no copy in between)
  leaves       names that are differentiable, `audio` first (the signal-like ones), then `controls` (small per-item tensors)
  same         {key: bound}: how equal two runs of the same computation must be - 0.0 (the default) is bit for bit, otherwise
               max|a - b| <= bound * max|b| (the op's documented not-fixed-order sums); keys are "y0", "y1", ... and "g_<leaf>"
  compare(keys, got, want) -> findings: got against want at the op's EXISTING parity bound (against the float64 reference, and a subset
               run against the all-leaves run); None: the `same` rule is all there is
  reference(seed, gys) -> {key: float64 array} or None
  lowp         audio leaves that may be bfloat16 / float16;  forms: {control: "vector" | "matrix"};  twice: (leaf, leaf) or None
  mutate       names of make() that C6 overwrites (default: every tensor)

Every check returns a list of findings (strings; empty = the contract holds) and appends (check, key, measured) to `rec`."""
import contextlib

import torch

INPLACE = "modified by an inplace operation"


class Spec:
    def __init__(self, name, make, call, leaves, audio=(), device="cpu", same=None, compare=None, reference=None, lowp=(), forms=None,
                 twice=None, mutate=None, plan=None, reaches=(), cite="", functions=None, f64_controls=True, groups=None, outs=None,
                 on_device=False):
        self.name, self.make, self.call, self.device = name, make, call, device
        self.leaves, self.audio = tuple(leaves), tuple(audio)
        self.controls = tuple(n for n in self.leaves if n not in self.audio)
        self.same = dict(same or {})
        self.compare, self.reference = compare, reference
        self.lowp, self.forms, self.twice, self.mutate = tuple(lowp), dict(forms or {}), twice, mutate
        self.plan = dict(plan or {})            # config.plan attributes of the entry (binding, forced segment lengths)
        self.reaches = tuple(reaches)           # autograd.Function classes / torch.ops.dasp ops the entry runs (completeness)
        self.groups = dict(groups or {})        # {key of the reference: the gradient keys it joins}, as compare() joins them
        self.outs = outs                        # seed -> [(shape, is complex)] of the outputs, known without running the op
        self.on_device = on_device              # the reference itself needs the device (the generated noise stream, written out)
        self.cite = cite                        # where the bounds are asserted today
        self.functions = functions              # () -> the Python autograd.Function classes of the entry, whose backward is watched
        self.f64_controls = f64_controls        # False: the op follows the dtype of its controls (no float32 audio beside them)

    def __repr__(self):
        return self.name


# ---- running a graph --------------------------------------------------------------------------------------------------------------------

def outputs(spec, t):
    y = spec.call(t)
    return tuple(y) if isinstance(y, (tuple, list)) else (y,)


def leafed(spec, seed, need, change=None):
    """make(seed) with requires_grad on the leaves in `need`; change(t) may replace tensors before they become leaves."""
    t = dict(spec.make(seed))
    if change is not None:
        change(t)
    for n in spec.leaves:
        if n in need:
            t[n] = t[n].detach().requires_grad_(True) if not t[n].requires_grad else t[n]
    return t


def upstream(outs, seed):
    g = torch.Generator(device="cpu").manual_seed(1000 + seed)
    gys = []
    for o in outs:
        v = torch.randn(o.shape, generator=g, dtype=torch.float64)
        if o.is_complex():
            v = torch.complex(v, torch.randn(o.shape, generator=g, dtype=torch.float64))
        gys.append(v.to(device=o.device, dtype=o.dtype))
    return gys


def sync(spec):
    if torch.device(spec.device).type == "cuda":
        torch.cuda.synchronize()


def watch_nodes(outs, log):
    """Hook every custom-Function node of the graph under `outs`: log one that hands a gradient to an input without an edge (one that needs none).
    Seen behind the node, so it holds for the C++ autograd Functions of torch.ops.dasp as well as for the Python ones."""
    nodes, stack = set(), [o.grad_fn for o in outs]
    while stack:
        fn = stack.pop()
        if fn is None or fn in nodes:
            continue
        nodes.add(fn)
        stack += [n for n, _ in fn.next_functions]
    for node in nodes:
        if "CppNode" not in node.name() and not hasattr(node, "_forward_cls"):
            continue                                # custom Functions only, C++ and Python (a built-in CatBackward hands every slice back)

        def hook(grad_inputs, grad_outputs, node=node):
            for i, ((nxt, _), g) in enumerate(zip(node.next_functions, grad_inputs)):
                if nxt is None and g is not None:
                    log.append(("needs", f"{node.name()} returns a gradient for input {i}, which needs none"))
        node.register_hook(hook)


def run(spec, seed, need=None, gys=None, change=None, gy_seed=0, use=None, node_log=None):
    """One forward and one backward: {"y<i>": output, "g_<leaf>": .grad or None}, plus the tensors under "_t" and the upstream gradients
    under "_gys". use: indices of the outputs the loss uses (None: all). node_log: see watch_nodes."""
    need = spec.leaves if need is None else need
    t = leafed(spec, seed, need, change)
    outs = outputs(spec, t)
    res = {"y%d" % i: o.detach() for i, o in enumerate(outs)}
    res["_t"], res["_outs"] = t, outs
    if need and node_log is not None:
        watch_nodes(outs, node_log)
    if need:
        gys = upstream(outs, gy_seed) if gys is None else gys
        idx = range(len(outs)) if use is None else use
        torch.autograd.backward([outs[i] for i in idx], [gys[i] for i in idx])
        res["_gys"] = gys
    for n in spec.leaves:
        res["g_" + n] = t[n].grad
    sync(spec)
    return res


def grad_keys(spec, need=None):
    return ["g_" + n for n in (spec.leaves if need is None else need)]


def rel(a, b):
    """max|a - b| / max|b| (0 / 0 = 0)."""
    if a is None or b is None or a.shape != b.shape:
        return float("inf")
    wide = torch.complex128 if a.is_complex() else torch.float64
    a, b = a.detach().to(wide), b.detach().to(wide)
    if a.numel() == 0:
        return 0.0
    d, m = float((a - b).abs().max()), float(b.abs().max())
    if d != d:
        return float("inf")
    return 0.0 if d == 0.0 else (d / m if m > 0.0 else float("inf"))


def same(spec, check, keys, got, want, rec, what="", rounding=0.0):
    """got[key] against want[key] by the spec's run-to-run rule. rounding: the epsilon of a low-precision dtype the values were rounded
    to - where the rule is not bit for bit, a float32 difference inside it may round to the neighbouring low-precision value."""
    out = []
    for k in keys:
        a, b = got.get(k), want.get(k)
        if a is None and b is None:
            continue
        e = rel(a, b)
        rec.append((check, k, e))
        bound = spec.same.get(k, 0.0)
        if bound > 0.0 and a is not None and a.dtype in (torch.bfloat16, torch.float16):
            bound += rounding
        if a is None or b is None or not bool(torch.isfinite(torch.view_as_real(a) if a.is_complex() else a.float()).all()):
            out.append(f"{check} {what} {k}: missing or non-finite")
        elif e > bound:
            out.append(f"{check} {what} {k}: differs by {e:.3e} of the largest entry (allowed: {'bit for bit' if bound == 0.0 else bound})")
    return out


def y_keys(res):
    return sorted(k for k in res if k.startswith("y"))


# ---- what backward() itself returns ------------------------------------------------------------------------------------------------------
# autograd hides two mistakes of a backward: a gradient returned for an input that needs none is dropped, and one of another dtype or of
# a broadcastable shape is cast / summed to the input's. Both are seen only where backward returns, so the Python Functions of an entry
# are wrapped while C1 and C5 run; C1 also hooks the nodes of the graph (watch_nodes), which sees the first mistake behind the C++
# twins too (the second is cast before a node hook runs: their like_control is read instead).

@contextlib.contextmanager
def watched(spec, log):
    """Wrap forward / backward of spec.functions(): log ("needs" | "form", message) for what autograd would hide, and ("entered", class
    name) for every forward that runs."""
    undo = []
    for cls in (spec.functions() if spec.functions else ()):
        f0, b0 = cls.__dict__.get("forward"), cls.__dict__.get("backward")
        if not isinstance(f0, staticmethod) or not isinstance(b0, staticmethod):
            continue

        def fwd(ctx, *args, _f=f0.__func__, _n=cls.__name__):
            log.append(("entered", _n))
            ctx._contract_meta = [(a.dtype, a.shape) if isinstance(a, torch.Tensor) else None for a in args]
            return _f(ctx, *args)

        def bwd(ctx, *grads, _b=b0.__func__, _n=cls.__name__):
            out = _b(ctx, *grads)
            outs = out if isinstance(out, tuple) else (out,)
            for i, (o, need, meta) in enumerate(zip(outs, ctx.needs_input_grad, ctx._contract_meta)):
                if o is not None and not need:
                    log.append(("needs", f"{_n}.backward returns a gradient for input {i}, which needs none"))
                elif o is not None and meta is not None and (o.dtype != meta[0] or o.shape != meta[1]):
                    log.append(("form", f"{_n}.backward returns {o.dtype} {tuple(o.shape)} for input {i}, a {meta[0]} {tuple(meta[1])}"))
            return out
        cls.forward, cls.backward = staticmethod(fwd), staticmethod(bwd)
        undo.append((cls, f0, b0))
    try:
        yield
    finally:
        for cls, f0, b0 in undo:
            cls.forward, cls.backward = f0, b0


def logged(log, kind, check):
    return sorted({f"{check} {msg}" for k, msg in log if k == kind})


# ---- C1: subsets of leaves --------------------------------------------------------------------------------------------------------------

def subsets(spec):
    """only the audio, only the controls, every control alone, every audio leaf alone (where there are several), everything."""
    out = []
    if spec.audio and spec.controls:
        out += [spec.audio, spec.controls]
    singles = [(n,) for n in spec.leaves]
    out += [s for s in singles if s not in out and len(spec.leaves) > 1]
    return out + [spec.leaves]


def check_subsets(spec, rec, seed=0):
    log = []
    with watched(spec, log):
        find = _check_subsets(spec, rec, seed, log)
    # completeness by running, not by name: every Python Function the entry claims to reach did run
    entered = {msg for kind, msg in log if kind == "entered"}
    find += [f"C1 the entry names {c.__name__}, whose forward never ran" for c in (spec.functions() if spec.functions else ()) if c.__name__ not in entered]
    return find + logged(log, "needs", "C1")


def _check_subsets(spec, rec, seed, log):
    find = []
    full = run(spec, seed)
    ys = y_keys(full)
    ref = spec.reference(seed, full["_gys"]) if spec.reference else None
    if ref is not None:
        find += spec.compare(ys + grad_keys(spec), full, ref, rec, "C1.all_vs_float64")
    for need in subsets(spec)[:-1]:
        what = "+".join(need)
        got = run(spec, seed, need=need, gys=full["_gys"], node_log=log)
        for n in spec.leaves:
            if n not in need and got["g_" + n] is not None:
                find.append(f"C1 [{what}] {n}: a gradient for a leaf that asked for none")
            if n in need and got["g_" + n] is None:
                find.append(f"C1 [{what}] {n}: no gradient")
        keys = [k for k in grad_keys(spec, need) if got[k] is not None]
        find += same(spec, "C1.y", ys, got, full, rec, f"[{what}]")
        if spec.compare:
            find += spec.compare(keys, got, full, rec, f"C1.subset_vs_all[{what}]")
            if ref is not None:            # (the gradients this subset did not ask for: the all-leaves run's, checked above)
                filled = {k: (got[k] if got.get(k) is not None else full[k]) for k in grad_keys(spec)}
                find += spec.compare(keys, filled, ref, rec, f"C1.subset_vs_float64[{what}]")
        else:
            find += same(spec, "C1.subset_vs_all", keys, got, full, rec, f"[{what}]")
    # no leaf requires a gradient, and grad mode off: a plain forward, same bits as the forward that saves
    for what, ctx in (("no leaf requires grad", contextlib.nullcontext()), ("no_grad", torch.no_grad())):
        with ctx:
            t = leafed(spec, seed, spec.leaves if what == "no_grad" else ())
            outs = outputs(spec, t)
        sync(spec)
        if any(o.requires_grad for o in outs):
            find.append(f"C1 {what}: the output requires grad")
        find += same(spec, "C1.plain_forward", ys, {"y%d" % i: o for i, o in enumerate(outs)}, full, rec, f"[{what}]")
    return find


# ---- C2: repeated backward --------------------------------------------------------------------------------------------------------------

def grads_of(spec, outs, t, gys):
    g = torch.autograd.grad(outs, [t[n] for n in spec.leaves], gys, retain_graph=True, allow_unused=True)
    sync(spec)
    return {"g_" + n: v for n, v in zip(spec.leaves, g)}


def check_repeat(spec, rec, seed=0):
    t = leafed(spec, seed, spec.leaves)
    outs = outputs(spec, t)
    gy, gy2 = upstream(outs, 0), upstream(outs, 1)
    first = grads_of(spec, outs, t, gy)
    second = grads_of(spec, outs, t, gy)
    other = grads_of(spec, outs, t, gy2)
    fourth = grads_of(spec, outs, t, gy)
    keys = grad_keys(spec)
    find = same(spec, "C2.second_vs_first", keys, second, first, rec) + same(spec, "C2.fourth_vs_first", keys, fourth, first, rec)
    alone = run(spec, seed, gys=gy2)
    return find + same(spec, "C2.other_gy_vs_fresh_graph", keys, other, alone, rec)


# ---- C3: interleaved graphs -------------------------------------------------------------------------------------------------------------

def check_interleave(spec, rec, seed=0):
    solo = [run(spec, seed + k) for k in (0, 1)]
    ta, tb = leafed(spec, seed, spec.leaves), leafed(spec, seed + 1, spec.leaves)
    oa = outputs(spec, ta)
    ob = outputs(spec, tb)
    torch.autograd.backward(ob, solo[1]["_gys"])
    torch.autograd.backward(oa, solo[0]["_gys"])
    sync(spec)
    find = []
    for tag, t, outs, ref in (("A", ta, oa, solo[0]), ("B", tb, ob, solo[1])):
        got = {"g_" + n: t[n].grad for n in spec.leaves}
        got.update({"y%d" % i: o.detach() for i, o in enumerate(outs)})
        find += same(spec, "C3.interleaved_vs_alone", y_keys(ref) + grad_keys(spec), got, ref, rec, f"[graph {tag}]")
    return find


# ---- C4: forms of the upstream gradient -------------------------------------------------------------------------------------------------

def _sliced(g):
    """g as a slice of a wider tensor: every second element of the last axis (a 0-dim g: one element of a longer buffer)."""
    if g.dim() == 0:
        buf = torch.full((5,), 7.0, dtype=g.dtype, device=g.device)
        buf[3] = g
        return buf[3]
    wide = torch.full(g.shape[:-1] + (2 * g.shape[-1] + 1,), 7.0, dtype=g.dtype, device=g.device)
    v = wide[..., 1::2]
    v.copy_(g)
    return v


def _channel_sliced(g):
    """g as the odd channels of a tensor with twice as many along axis 1 (needs two axes)."""
    if g.dim() < 2:
        return _sliced(g)
    shape = list(g.shape)
    shape[1] = 2 * shape[1] + 1
    wide = torch.full(shape, 7.0, dtype=g.dtype, device=g.device)
    v = wide[:, 1::2]
    v.copy_(g)
    return v


def _transposed(g):
    if g.dim() < 2:
        return _sliced(g)
    return g.transpose(0, -1).contiguous().transpose(0, -1)


def check_upstream_forms(spec, rec, seed=0):
    find = []
    base = run(spec, seed)
    gys, keys = base["_gys"], grad_keys(spec)
    n_out = len(gys)
    # .sum().backward(): an expanded scalar, stride 0
    ones = run(spec, seed, gys=[torch.ones_like(g) for g in gys])
    t = leafed(spec, seed, spec.leaves)
    outs = outputs(spec, t)
    sum(o.sum() if not o.is_complex() else torch.view_as_real(o)[..., 0].sum() for o in outs).backward()
    sync(spec)
    find += same(spec, "C4.sum_backward_vs_ones", keys, {"g_" + n: t[n].grad for n in spec.leaves}, ones, rec)
    # views: every upstream gradient non-contiguous at once (several outputs: each must be the one the kernel reads)
    for tag, view in (("last_axis_slice", _sliced), ("channel_slice", _channel_sliced), ("transposed", _transposed)):
        vs = [view(g) for g in gys]
        if all(v.is_contiguous() and v.storage_offset() == 0 for v in vs):
            continue
        assert all(torch.equal(v, g) for v, g in zip(vs, gys))
        find += same(spec, "C4." + tag, keys, run(spec, seed, gys=vs), base, rec)
    # exact zeros
    zero = run(spec, seed, gys=[torch.zeros_like(g) for g in gys])
    for k in keys:
        g = zero[k]
        if g is None or bool((torch.view_as_real(g) if g.is_complex() else g).ne(0).any()) or not bool(torch.isfinite(torch.view_as_real(g) if g.is_complex() else g).all()):
            find.append(f"C4.zero_gy {k}: not exactly zero")
    # several outputs: a loss on one of them == explicit zeros for the others
    if n_out > 1:
        for i in range(n_out):
            padded = run(spec, seed, gys=[g if j == i else torch.zeros_like(g) for j, g in enumerate(gys)])
            find += same(spec, "C4.one_output_vs_zeros", keys, run(spec, seed, gys=gys, use=[i]), padded, rec, f"[output {i}]")
    return find


# ---- C5: dtypes, shapes and layouts of the leaves ---------------------------------------------------------------------------------------

def _as_leaf_views(forms, kind):
    """change(t) that hands the controls over in another form with the same values."""
    def change(t):
        for n, f in forms.items():
            c = t[n]
            if kind == "float64":
                t[n] = c.double()
            elif kind == "strided":
                wide = torch.full(c.shape + (3,), 7.0, dtype=c.dtype, device=c.device)
                wide[..., 1] = c
                t[n] = wide[..., 1]
                assert c.numel() < 2 or not t[n].is_contiguous()
            elif kind == "layout" and f == "matrix" and c.dim() >= 2:
                t[n] = c.transpose(0, -1).contiguous().transpose(0, -1)
            elif f == "vector" and kind in ("flat", "col", "col1"):
                t[n] = c.reshape({"flat": (-1,), "col": (-1, 1), "col1": (-1, 1, 1)}[kind]).clone()
            elif f == "vector" and kind == "expand":
                t[n] = c.reshape(-1)[:1].clone().expand(c.numel())
    return change


def check_leaf_forms(spec, rec, seed=0):
    log = []
    with watched(spec, log):
        find = _check_leaf_forms(spec, rec, seed)
    return find + logged(log, "form", "C5")


def _check_leaf_forms(spec, rec, seed=0):
    find = []
    base = run(spec, seed)
    ys, keys = y_keys(base), grad_keys(spec)
    for n in spec.leaves:
        g, leaf = base["g_" + n], base["_t"][n]
        rec.append(("C5.dtype_shape_device", "g_" + n, float(g is None or g.dtype != leaf.dtype or g.shape != leaf.shape or g.device != leaf.device)))
        if g is None or g.dtype != leaf.dtype or g.shape != leaf.shape or g.device != leaf.device:
            find.append(f"C5 g_{n}: {None if g is None else (g.dtype, tuple(g.shape), g.device)} for a leaf {(leaf.dtype, tuple(leaf.shape), leaf.device)}")
    # low-precision audio: the float32 run on the rounded input, rounded once
    for dt in (torch.bfloat16, torch.float16):
        if not spec.lowp:
            break
        eps = torch.finfo(dt).eps

        def lower(t, dt=dt):
            for n in spec.lowp:
                t[n] = t[n].to(dt)

        def rounded(t, dt=dt):
            for n in spec.lowp:
                t[n] = t[n].to(dt).float()
        got = run(spec, seed, change=lower)                      # (its upstream gradients are drawn in the outputs' dtype)
        want = run(spec, seed, change=rounded, gys=[g.float() if g.dtype == dt else g for g in got["_gys"]])
        for k in ys + keys:
            a, b = got[k], want[k]
            is_lo = b is not None and b.dtype == torch.float32 and (k[2:] in spec.lowp if k.startswith("g_") else True)
            if a is None or b is None or a.dtype != (dt if is_lo else b.dtype) or a.shape != b.shape:
                find.append(f"C5 {dt} {k}: {None if a is None else (a.dtype, tuple(a.shape))}")
                continue
            e = rel(a, b)
            rec.append(("C5.%s" % str(dt).split(".")[1], k, e))
            a, b = a.double(), b.double()
            # (one rounding: eps of the value, or one step of the dtype's subnormals)
            allowed = (eps * b.abs() + eps * torch.finfo(dt).smallest_normal if is_lo else 0.0) + spec.same.get(k, 0.0) * float(b.abs().max())
            if not bool(((a - b).abs() <= allowed).all()):
                find.append(f"C5 {dt} {k}: {e:.3e} of the largest entry from the float32 run on the rounded input (allowed: one rounding, {eps:.1e} per element)")
    # the controls in other shapes, layouts and dtypes: the values of the contiguous float32 case
    kinds = (["float64"] if spec.f64_controls else []) + ["strided"] + (["flat", "col", "col1", "expand"] if "vector" in spec.forms.values() else []) \
        + (["layout"] if "matrix" in spec.forms.values() else [])
    for kind in kinds if spec.forms else []:
        change = _as_leaf_views(spec.forms, kind)
        want = base
        if kind == "expand":            # one value for every item: compare with the contiguous tensor of those values
            def flat_same(t):
                for n, f in spec.forms.items():
                    if f == "vector":
                        t[n] = t[n].reshape(-1)[:1].expand(t[n].numel()).reshape(t[n].shape).clone()
            want = run(spec, seed, change=flat_same, gys=base["_gys"])
        got = run(spec, seed, change=change, gys=base["_gys"])
        for n in spec.forms:
            g, leaf = got["g_" + n], got["_t"][n]
            if g is None or g.dtype != leaf.dtype or g.shape != leaf.shape:
                find.append(f"C5 [{kind}] g_{n}: {None if g is None else (g.dtype, tuple(g.shape))} for a leaf {(leaf.dtype, tuple(leaf.shape))}")
                continue
            got["g_" + n] = g.reshape(want["g_" + n].shape).to(want["g_" + n].dtype)
        find += same(spec, "C5.control_form", ys + keys, got, want, rec, f"[{kind}]")
    # one leaf passed twice: its .grad is the sum of the two gradients
    if spec.twice:
        a, b = spec.twice

        def both_a(t):
            t[b] = t[a].clone()
        apart = run(spec, seed, change=both_a, gys=base["_gys"])
        t = leafed(spec, seed, [n for n in spec.leaves if n != b])
        t[b] = t[a]
        outs = outputs(spec, t)
        torch.autograd.backward(outs, base["_gys"])
        sync(spec)
        want = {k: apart[k] for k in keys}                 # (the other leaves, as a grouped bound needs them: the two runs' own)
        got = {k: (t[k[2:]].grad if k[2:] != b else apart[k]) for k in keys}
        want["g_" + a] = apart["g_" + a] + apart["g_" + b]
        if spec.compare:
            find += spec.compare(["g_" + a], got, want, rec, f"C5.leaf_twice[{a}={b}]")
        else:
            find += same(spec, "C5.leaf_twice", ["g_" + a], got, want, rec, f"[{a}={b}]")
    return find


# ---- C6: mutation between forward and backward ------------------------------------------------------------------------------------------

def check_mutation(spec, rec, seed=0):
    find = []

    def strided_audio(t):
        for n in spec.audio:
            x = t[n]
            wide = torch.full(x.shape[:-1] + (x.shape[-1] + 21,), 7.0, dtype=x.dtype, device=x.device)
            wide[..., 9:9 + x.shape[-1]] = x
            t[n] = wide[..., 9:9 + x.shape[-1]]

    def low_audio(t):
        for n in spec.lowp:
            t[n] = t[n].to(torch.bfloat16)
    variants = [("as_is", None)] + ([("strided_audio", strided_audio)] if spec.audio else []) + ([("bf16_audio", low_audio)] if spec.lowp else [])
    for tag, change in variants:
        base = run(spec, seed, change=change)
        names = [n for n, v in base["_t"].items() if isinstance(v, torch.Tensor)] if spec.mutate is None else list(spec.mutate)
        donor = dict(spec.make(seed + 1))
        if change is not None:
            change(donor)
        for name in names:
            t = leafed(spec, seed, spec.leaves, change)
            outs = outputs(spec, t)
            with torch.no_grad():
                if t[name].is_floating_point() or t[name].is_complex():
                    new = donor[name].to(t[name].dtype)
                    t[name].copy_(torch.where(new == t[name], new + 1, new) if not new.is_complex() else new + 1)
                else:
                    t[name].add_(1)
            try:
                torch.autograd.backward(outs, base["_gys"])
                sync(spec)
            except RuntimeError as e:
                if INPLACE not in str(e):
                    raise
                rec.append(("C6.raises", f"{tag}:{name}", 1.0))
                continue
            rec.append(("C6.raises", f"{tag}:{name}", 0.0))
            got = {"g_" + n: t[n].grad for n in spec.leaves}
            find += same(spec, "C6.gradient_of_what_the_forward_saw", grad_keys(spec), got, base, rec, f"[{tag}, {name} overwritten]",
                         rounding=torch.finfo(torch.bfloat16).eps)
    return find


# ---- C7: streams ------------------------------------------------------------------------------------------------------------------------

def check_streams(spec, rec, seed=0):
    base = run(spec, seed)
    t = leafed(spec, seed, spec.leaves)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=spec.device)
    with torch.cuda.stream(side):
        outs = outputs(spec, t)
    torch.cuda.current_stream().wait_stream(side)
    torch.autograd.backward(outs, base["_gys"])
    torch.cuda.synchronize()
    got = {"g_" + n: t[n].grad for n in spec.leaves}
    got.update({"y%d" % i: o.detach() for i, o in enumerate(outs)})
    return same(spec, "C7.side_stream_forward", y_keys(base) + grad_keys(spec), got, base, rec)


CHECKS = {"C1_subsets": check_subsets, "C2_repeat": check_repeat, "C3_interleave": check_interleave, "C4_upstream_forms": check_upstream_forms,
          "C5_leaf_forms": check_leaf_forms, "C6_mutation": check_mutation, "C7_streams": check_streams}
