from .checkpoints import *  # noqa: F401,F403
from .fit import *          # noqa: F401,F403
from .device import *  # noqa: F401,F403
from .seed import *    # noqa: F401,F403
from .frozen_bn import *  # noqa: F401,F403
from ..ema import ModelEMA  # noqa: F401
