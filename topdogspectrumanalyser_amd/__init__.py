"""topdogspectrumanalyser_amd - MI355X-native "sample method" IQ -> spectrum path.

Hand-written HIP (gfx950) kernels behind a ctypes C-ABI (include/tdsa_hip.h), kept behind the
reference's own SampleDataSource / DataProcessor Python API.  Importing the package requires
libtdsa_hip.so (built by __graft_entry__.build()); there is no CPU fallback.
"""
from .devmem import DeviceBuffer  # noqa: F401
from .engine import HostPipe, SpectrumEngine, TraceState  # noqa: F401
from .utils.signal_processing import TraceAverager  # noqa: F401
from .datasources import (SOURCE_CLASSES, HackrfSamplesDataSource, MicrophoneSamplesDataSource,  # noqa: F401
                          RtlSamplesDataSource, SampleDataSource, SweepDataSource)
from .core.display_data_processor import DataProcessor  # noqa: F401
from .core.tare_state import TareState  # noqa: F401
from .analytics import Constellation, ConstellationView  # noqa: F401
from .zoom import DownConverter, ZoomSpectrum, design_decimator  # noqa: F401
from .channelizer import Channelizer, ChannelSpectra  # noqa: F401
from .demod import Demodulator, deemphasis_pole, design_audio_filter  # noqa: F401
from .symbols import SymbolSync, rrc_taps  # noqa: F401
from .fsk import FskAnalyzer, FskResult  # noqa: F401
from .eye import EyeDiagram, EyeImage  # noqa: F401
from .modquality import ModQResult, ModQuality  # noqa: F401
from .detect import Detections, SignalDetector  # noqa: F401
from .measure import ChannelMeasure, Measurements, channel_plan, channels_from_emission, limit_line  # noqa: F401
from .powerstats import PowerStatistics, PowerStats, gaussian_ccdf  # noqa: F401
from .pulses import PulseAnalyzer, PulseTrain, levels_from_db  # noqa: F401
from .correlate import Correlator, Matches, barker, from_symbols, zadoff_chu  # noqa: F401
from .zerospan import ZeroSpan, view_plan  # noqa: F401
from .history3d import RibbonView, SurfaceView, ThreeDView, TraceHistory  # noqa: F401
from .sweep import IqSweepDataSource, SweepAssembler, plan_steps  # noqa: F401

__all__ = ["DeviceBuffer", "SpectrumEngine", "HostPipe", "TraceState", "TraceAverager", "SampleDataSource", "SweepDataSource",
           "HackrfSamplesDataSource", "RtlSamplesDataSource", "MicrophoneSamplesDataSource",
           "SOURCE_CLASSES", "DataProcessor", "TareState", "Constellation", "ConstellationView",
           "DownConverter", "ZoomSpectrum", "design_decimator", "ZeroSpan", "view_plan", "IqSweepDataSource", "SweepAssembler", "plan_steps",
           "TraceHistory", "RibbonView", "ThreeDView", "SurfaceView", "Channelizer", "ChannelSpectra",
           "Demodulator", "design_audio_filter", "deemphasis_pole", "SignalDetector", "Detections", "ChannelMeasure", "Measurements",
           "channel_plan", "limit_line", "channels_from_emission", "PowerStats", "PowerStatistics", "gaussian_ccdf",
           "PulseAnalyzer", "PulseTrain", "levels_from_db", "Correlator", "Matches", "zadoff_chu", "barker", "from_symbols", "FskAnalyzer", "FskResult",
           "EyeDiagram", "EyeImage", "ModQuality", "ModQResult"]
