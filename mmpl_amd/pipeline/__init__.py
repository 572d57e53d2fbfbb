from .casual_fps_inference import CausalFPSInferencePipeline  # noqa: F401
from .causal_inference import CausalInferencePipeline  # noqa: F401
