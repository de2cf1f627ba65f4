"""Shim package: ``utils`` of the reference's demos/yolov3_huaweiShip (train.py:11-12,16; inference.py:21)."""
from fastvision_amd.demos.yolov3_huaweiShip.utils import *  # noqa: F401,F403
from fastvision_amd.demos.yolov3_huaweiShip.utils import ComputeLoss, grid, mean_average_precision, non_max_suppression, non_max_suppression_batch, xywh2xyxy  # noqa: F401
