"""Shim package: ``cfg`` of the reference's demos/yolov3_huaweiShip (train.py:13 ``from cfg._fit import Fit``)."""
