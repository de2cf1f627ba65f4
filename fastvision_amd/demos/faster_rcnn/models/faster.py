"""The reference's Faster R-CNN demo model on the HIP ops -- API mirror of demos/faster_rcnn/models/faster.py (class Faster_Rcnn:
same constructor arguments, sub-module names ``backbone`` / ``rpn`` / ``fast`` and return values).

    images [B,3,H,W] -> VGG16 (stride 16) -> RPN (proposals; training: its two losses) -> Fast head (training: its two losses;
    inference: per-image detections [n, 6] = xywh in feature cells, class, score)

``detect`` (not in the reference): the same inference for the whole batch -- one heads pass, one decode launch, one batched NMS ->
padded detections in pixels on the device (what ``cfg._fit.Validate`` and ``inference.Inference(batch_size > 1)`` call).

``perms``: optional list of 2*B (perm_pos, perm_neg) pairs -- the RPN's per image, then the Fast head's -- instead of
``torch.randperm`` draws (parity tests share the reference's).
"""
import torch
import torch.nn as nn

from ....detect_ops import NMS_DEMO, nms_batch_padded
from .fast import Fast
from .rpn import RPN
from .vgg import vgg16

__all__ = ['Faster_Rcnn']


class Faster_Rcnn(nn.Module):
    def __init__(self, training=False, in_channels=3, num_classes=80, base_anchors=None, backbone_stride=16, backbone_output_channels=512,
                 backbone_weights='', rpn_positive_iou_thres=0.7, rpn_negative_iou_thres=0.3, rpn_positives_per_image=128,
                 rpn_negatives_per_image=128, rpn_pre_nms_top_n=2000, rpn_post_nms_top_n=2000, rpn_nms_thresh=0.7, fast_multi_reg_head=False,
                 fast_positive_iou_thres=0.5, fast_negative_iou_thres=0.5, fast_positives_per_image=16, fast_negatives_per_image=48,
                 fast_roi_pool=7):
        super().__init__()
        self.training = training
        self.backbone_stride = backbone_stride
        self.backbone = vgg16(in_channels=in_channels)
        if backbone_weights:
            have, own = torch.load(backbone_weights), self.backbone.state_dict()
            matched = {k: v for k, v in have.items() if k in own and v.size() == own[k].size()}
            self.backbone.load_state_dict(matched, strict=False)
            print('Backbone not matched keys : ', [k for k in have if k not in matched])
        self.rpn = RPN(training=training, base_anchors=base_anchors, backbone_stride=backbone_stride, in_channels=backbone_output_channels,
                       rpn_pre_nms_top_n=rpn_pre_nms_top_n, rpn_post_nms_top_n=rpn_post_nms_top_n, rpn_nms_thresh=rpn_nms_thresh,
                       rpn_positive_iou_thres=rpn_positive_iou_thres, rpn_negative_iou_thres=rpn_negative_iou_thres,
                       rpn_positives_per_image=rpn_positives_per_image, rpn_negatives_per_image=rpn_negatives_per_image)
        self.fast = Fast(training=training, fast_multi_reg_head=fast_multi_reg_head, module_after_roi=self.backbone.classifier,
                         in_channels=backbone_output_channels, num_classes=num_classes, fast_positive_iou_thres=fast_positive_iou_thres,
                         fast_negative_iou_thres=fast_negative_iou_thres, fast_positives_per_image=fast_positives_per_image,
                         fast_negatives_per_image=fast_negatives_per_image, fast_roi_pool=fast_roi_pool)

    def forward(self, images, targets=None, perms=None):
        feature_backbone = self.backbone(images)
        if self.training:
            n = images.size(0)
            proposals, loss_rpn_cls, loss_rpn_box = self.rpn(feature_backbone, targets, perms=perms[:n] if perms else None)
            loss_fast_cls, loss_fast_box = self.fast(feature_backbone, proposals, targets, perms=perms[n:] if perms else None)
            return proposals, loss_rpn_cls, loss_rpn_box, loss_fast_cls, loss_fast_box
        return self.fast(feature_backbone, self.rpn(feature_backbone))

    def detect(self, images, conf_thres, iou_thres, max_det=300, letterboxes=None):
        """Batched evaluation (not in the reference, which post-processes image by image): backbone -> RPN -> Fast.detect (one heads
        pass, one decode launch) -> per-class NMS of the whole batch.  -> (dets [B, max_det, 6] = x1, y1, x2, y2, score, category, best
        score first; kept [B] int32), both on the device: image b's detections are dets[b, :kept[b]] -- what
        metrics.CalculateMAP.process_batch takes.  Boxes are in input pixels, or in each image's original frame when ``letterboxes``
        (per image resize_ratio, pad_left, pad_top, ori_w, ori_h) is given.  Host read-backs: the ones the RPN's and this NMS's
        candidate counts already are."""
        if self.training:
            raise RuntimeError('Faster_Rcnn.detect: the model is in training mode; call eval() first')
        feature_backbone = self.backbone(images)
        pred = self.fast.detect(feature_backbone, self.rpn(feature_backbone), self.backbone_stride, tuple(images.shape[2:]), letterboxes)
        dets, _, kept = nms_batch_padded(pred, conf_thres, iou_thres, max_det, NMS_DEMO)
        return dets, kept
