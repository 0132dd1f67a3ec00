"""The maintainer-side patch of INTEGRATION.md section 3, executed: the code block is taken from the document itself, run in front of
the package's own __init__.py (as the text says a maintainer would place it), and the resulting package is checked - every Processor
routes device tensors to the dasp_pytorch_amd functions and CPU tensors to the package's own code.

The package is a stand-in written by the test: laid out as the reference's dasp_pytorch is (functional / signal / modules, modules
binding the functions by name at import, Processor.process_fn, process_normalized denormalising by param_ranges and passing keywords,
__init__ importing functional before modules), with its CPU paths computed by the numpy oracle and the parameter ranges of
dasp_pytorch_amd.modules (the mirror of the reference's). So the test needs nothing outside the repository."""
import os
import re
import sys
import textwrap
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STAND_IN = {
    "__init__.py": """
        from dasp_pytorch.functional import (gain, stereo_bus, stereo_panner, stereo_widener, noise_shaped_reverberation, compressor,
                                             distortion, parametric_eq)
        from dasp_pytorch.modules import Processor, Compressor, ParametricEQ, NoiseShapedReverb, Gain, Distortion
        """,
    "functional.py": """
        import numpy as np
        import torch

        from oracle import dasp_oracle as _orc


        def _np(t):
            return t.detach().cpu().double().numpy()


        def _cpu_only(name):
            def fn(*a, **k):
                raise NotImplementedError(f"stand-in: the CPU path of {name} is not part of the test")
            return fn


        def gain(x, sample_rate, gain_db):
            return torch.from_numpy(_orc.gain(_np(x), sample_rate, _np(gain_db))).to(x.dtype)


        def distortion(x, sample_rate, drive_db):
            return torch.from_numpy(_orc.distortion(_np(x), sample_rate, _np(drive_db))).to(x.dtype)


        def parametric_eq(x, sample_rate, *bands, **named):          # the 18 controls in the reference's argument order
            params = torch.stack([torch.as_tensor(c) for c in list(bands) + list(named.values())], 1)
            return torch.from_numpy(_orc.parametric_eq(_np(x), sample_rate, _np(params))).to(x.dtype)


        compressor = _cpu_only("compressor")
        noise_shaped_reverberation = _cpu_only("noise_shaped_reverberation")
        stereo_widener = _cpu_only("stereo_widener")
        stereo_panner = _cpu_only("stereo_panner")
        stereo_bus = _cpu_only("stereo_bus")
        """,
    "signal.py": """
        from dasp_pytorch.functional import _cpu_only

        sosfilt_via_fsm = _cpu_only("sosfilt_via_fsm")
        lfilter_via_fsm = _cpu_only("lfilter_via_fsm")
        biquad = _cpu_only("biquad")
        """,
    "modules.py": """
        from dasp_pytorch.functional import gain, distortion, parametric_eq, compressor, noise_shaped_reverberation

        import dasp_pytorch_amd.modules as _amd


        class Processor:
            def __init__(self, sample_rate, process_fn, ranges_of):
                self.sample_rate = sample_rate
                self.process_fn = process_fn
                self.param_ranges = ranges_of(sample_rate).param_ranges

            def process_normalized(self, x, param_tensor):
                p = {k: lo + param_tensor[:, i] * (hi - lo) for i, (k, (lo, hi)) in enumerate(self.param_ranges.items())}
                return self.process_fn(x, self.sample_rate, **p)

            def process(self, x, *args):
                return self.process_fn(x, *args)


        class Gain(Processor):
            def __init__(self, sample_rate):
                super().__init__(sample_rate, gain, _amd.Gain)


        class Distortion(Processor):
            def __init__(self, sample_rate):
                super().__init__(sample_rate, distortion, _amd.Distortion)


        class ParametricEQ(Processor):
            def __init__(self, sample_rate):
                super().__init__(sample_rate, parametric_eq, _amd.ParametricEQ)


        class Compressor(Processor):
            def __init__(self, sample_rate):
                super().__init__(sample_rate, compressor, _amd.Compressor)


        class NoiseShapedReverb(Processor):
            def __init__(self, sample_rate):
                super().__init__(sample_rate, noise_shaped_reverberation, _amd.NoiseShapedReverb)
        """,
}


def _write_stand_in(root):
    pkg = os.path.join(root, "dasp_pytorch")
    os.makedirs(pkg)
    for name, src in STAND_IN.items():
        with open(os.path.join(pkg, name), "w") as f:
            f.write(textwrap.dedent(src).lstrip())
    return pkg


def _stub_source():
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = md[md.index("## 3. Patch inside the reference"):md.index("## 4.")]
    return re.search(r"```python\n(.*?)```", sec, re.S).group(1)


def test_integration_stub_routes_processors(monkeypatch, tmp_path):
    if torch.version.hip is None:
        pytest.skip("the stub is conditional on a ROCm build of torch")
    REF = _write_stand_in(str(tmp_path))
    import dasp_pytorch_amd.functional as amd_f
    import dasp_pytorch_amd.signal as amd_s
    seen = []
    for mod, names in ((amd_f, ("gain", "distortion", "parametric_eq", "compressor", "noise_shaped_reverberation", "stereo_widener",
                                "stereo_panner", "stereo_bus")), (amd_s, ("sosfilt_via_fsm", "lfilter_via_fsm", "biquad"))):
        for n in names:
            monkeypatch.setattr(mod, n, (lambda n: lambda *a, **k: seen.append(n) or ("amd", n))(n))
    saved = {k: v for k, v in sys.modules.items() if k == "dasp_pytorch" or k.startswith("dasp_pytorch.")}
    for k in saved:
        del sys.modules[k]
    try:
        pkg = types.ModuleType("dasp_pytorch")
        pkg.__path__ = [REF]
        pkg.__package__ = "dasp_pytorch"
        pkg.__file__ = os.path.join(REF, "__init__.py")
        sys.modules["dasp_pytorch"] = pkg
        exec(compile(_stub_source(), "INTEGRATION.md#3", "exec"), pkg.__dict__)                       # the maintainer's block first ...
        exec(compile(open(pkg.__file__).read(), pkg.__file__, "exec"), pkg.__dict__)                  # ... then the reference's __init__

        class DeviceTensor:          # stands in for a tensor on the GPU (there is none here): the stub only looks at .is_cuda
            is_cuda = True
        SR = 44100
        eq, comp, rev, gain = pkg.ParametricEQ(SR), pkg.Compressor(SR), pkg.NoiseShapedReverb(SR), pkg.Gain(SR)
        for proc, name in ((eq, "parametric_eq"), (comp, "compressor"), (rev, "noise_shaped_reverberation"), (gain, "gain")):
            assert proc.process_fn(DeviceTensor(), SR) == ("amd", name)
        assert pkg.signal.sosfilt_via_fsm(None, DeviceTensor()) == ("amd", "sosfilt_via_fsm")
        assert pkg.signal.lfilter_via_fsm(DeviceTensor(), None) == ("amd", "lfilter_via_fsm")
        assert pkg.signal.biquad(DeviceTensor(), None, None, SR) == ("amd", "biquad")
        assert pkg.functional.stereo_bus(DeviceTensor(), SR, None) == ("amd", "stereo_bus")
        assert seen == ["parametric_eq", "compressor", "noise_shaped_reverberation", "gain", "sosfilt_via_fsm", "lfilter_via_fsm", "biquad",
                        "stereo_bus"]
        # CPU tensors keep the reference's own path, through the same Processor objects (process_normalized passes keywords)
        x = torch.rand(2, 1, 256) * 2 - 1
        y = gain.process_normalized(x, torch.tensor([[0.5], [1.0]]))
        assert torch.allclose(y[0], x[0]) and torch.allclose(y[1], x[1] * 10 ** (24 / 20), rtol=1e-5)
        y = eq.process_normalized(x, torch.rand(2, 18))
        assert y.shape == x.shape and torch.isfinite(y).all() and len(seen) == 8
    finally:
        for k in [k for k in sys.modules if k == "dasp_pytorch" or k.startswith("dasp_pytorch.")]:
            del sys.modules[k]
        sys.modules.update(saved)
