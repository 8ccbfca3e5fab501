"""MI355X-native EEG imagined-speech LSTM path (drop-in for the reference's Utilities package surface).

Public names mirror the reference: EEG_LSTM, SimplePredictor, CLASS_NAMES (Utilities/lstm_eeg_model.py),
run_trials, TrialResult (Utilities/tester.py), StreamingProcess (Utilities/streaming_process.py).
"""
from ._lib import NsdError, build as build_library, lib as load_library
from .lstm_eeg_model import CLASS_NAMES, EEG_LSTM, IdentityPreProcessor, SimplePredictor, resolve_reference_preprocessor
from .multimodel import EnsemblePredictor, ModelBatchTrainer
from .ops import Augment, Average, Crop, Loss, LrSchedule, ModelSpec, Sam
from .prep import CausalPrep
from .resample import Resample
from .gate import SignalGate
from .align import EnsembleSpatialFit, SessionAlign, SpatialFit
from .calibrate import HeadFit
from .stream import EnsembleSlidingStreamDecoder, EnsembleStreamDecoder, PredictorSlidingStream, PredictorStream, SlidingStreamDecoder, StreamDecoder
from .streaming_process import StreamingProcess
from .tester import DEFAULT_MODEL, DEFAULT_SERIAL, TrialResult, run_trials

__all__ = ["EEG_LSTM", "SimplePredictor", "CLASS_NAMES", "run_trials", "TrialResult", "StreamingProcess",
           "ModelSpec", "Augment", "Average", "Crop", "Sam", "Loss", "LrSchedule", "CausalPrep", "Resample", "SignalGate", "SessionAlign", "SpatialFit", "EnsembleSpatialFit", "HeadFit", "ModelBatchTrainer", "EnsemblePredictor", "StreamDecoder", "EnsembleStreamDecoder", "SlidingStreamDecoder", "EnsembleSlidingStreamDecoder", "PredictorStream", "PredictorSlidingStream", "NsdError", "IdentityPreProcessor", "resolve_reference_preprocessor", "build_library", "load_library", "DEFAULT_MODEL", "DEFAULT_SERIAL"]
