"""`models.darknet` of the ship demo is the yolov3_u module (byte-identical in the reference): the same module object, no second copy."""
import importlib
import sys

sys.modules[__name__] = importlib.import_module('fastvision_amd.demos.yolov3_u.models.darknet')
