from .darknet53 import *  # noqa: F401,F403  (mirrors classfication/models/__init__.py of the reference)
from .vgg import *  # noqa: F401,F403
from .resnext import *  # noqa: F401,F403  (before .resnet, as in the reference: the package-level ResNet / Bottleneck / BasicBlock stay resnet.py's)
from .resnet import *  # noqa: F401,F403
