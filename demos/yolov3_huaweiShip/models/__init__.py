"""Shim package: ``models`` of the reference's demos/yolov3_huaweiShip (train.py:14 ``from models.yolov3 import YoloV3``)."""
from fastvision_amd.demos.yolov3_huaweiShip.models import *  # noqa: F401,F403
from fastvision_amd.demos.yolov3_huaweiShip.models import YoloV3, darknet53  # noqa: F401
