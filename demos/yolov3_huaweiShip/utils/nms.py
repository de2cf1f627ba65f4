"""Shim: `utils.nms` of the reference's demos/yolov3_huaweiShip resolves to `fastvision_amd.demos.yolov3_huaweiShip.utils.nms` (the same module object)."""
import importlib
import sys

sys.modules[__name__] = importlib.import_module('fastvision_amd.demos.yolov3_huaweiShip.utils.nms')
