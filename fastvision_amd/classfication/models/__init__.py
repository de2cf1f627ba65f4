from .darknet53 import *  # noqa: F401,F403  (mirrors classfication/models/__init__.py of the reference)
from .vgg import *  # noqa: F401,F403
from .resnet import *  # noqa: F401,F403
