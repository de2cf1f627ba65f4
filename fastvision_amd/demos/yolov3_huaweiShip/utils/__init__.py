from .lossv3 import ComputeLoss  # noqa: F401
from ...yolov3_u.utils import grid, mean_average_precision, non_max_suppression, non_max_suppression_batch, xywh2xyxy  # noqa: F401
