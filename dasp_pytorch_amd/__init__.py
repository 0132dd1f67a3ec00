"""dasp_pytorch_amd -- MI355X-native hot path of dasp_pytorch.functional."""
from . import chain, config, functional, losses, modules, signal  # noqa: F401
from .functional import (advanced_distortion, ballistics, block_level, compressor, distortion, envelope_follower, expander, fdn_reverb, feedback_delay, gain, gain_curve, graphic_eq, limiter, loudness, loudness_normalize,  # noqa: F401
                         modulated_delay, noise_shaped_reverberation, oversampled_distortion, parametric_eq, peak_normalize, phaser, resample, sidechain_compressor, stereo_bus, stereo_mix, stereo_panner,
                         stereo_widener, time_varying_eq, time_varying_filter)
from .modules import (Compressor, Distortion, Expander, FDNReverb, FeedbackDelay, Gain, GainCurve, Limiter, ModulatedDelay, NoiseShapedReverb, OversampledDistortion, ParametricEQ, Phaser, Processor,  # noqa: F401
                      Resample, SidechainCompressor, TimeVaryingEQ, TimeVaryingFilter)
from .signal import control_frames, fdn_delay_lengths, resample_taps  # noqa: F401
