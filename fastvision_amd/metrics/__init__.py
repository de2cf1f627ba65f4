from .map import *        # noqa: F401,F403
from .accuracy import *   # noqa: F401,F403
