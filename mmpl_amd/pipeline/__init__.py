from .bidirectional_diffusion_inference import BidirectionalDiffusionInferencePipeline  # noqa: F401
from .bidirectional_inference import BidirectionalInferencePipeline  # noqa: F401
from .casual_fps_inference import CausalFPSInferencePipeline  # noqa: F401
from .causal_inference import CausalInferencePipeline  # noqa: F401
