from ...yolov3_u.models import YoloV3, darknet53  # noqa: F401
