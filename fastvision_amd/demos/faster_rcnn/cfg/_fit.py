"""Fit loop of the reference's Faster R-CNN demo -- API mirror of demos/faster_rcnn/cfg/_fit.py (clip_gradient, Fit, _Train).

Step contract (_fit.py:35-50): losses = model(images, targets); optimizer.zero_grad(); loss = the four losses summed;
loss.backward(); clip_gradient(model, 10.) ("for vgg only"); optimizer.step(); the learning rate is divided by ten at every ninth
epoch (:22-24) and the model's state_dict is saved after each epoch (:30).  Differences: the batch goes to the GPU here (the
reference leaves its .cuda() calls commented out and relies on DataParallel), the global norm is computed on the device with one
read-back instead of one per parameter, and the per-batch print reads the five loss values back in one transfer.  An optimizer
that clips by itself (``clip_norm`` set, e.g. fastvision_amd.FusedSGD(..., clip_norm=10.): norm and coefficient on the device, no
read-back) replaces the clip_gradient call.

``Validate`` (the reference's Fit takes a validation_loader and never uses it): mAP over a loader with the batched device path --
Faster_Rcnn.detect and CalculateMAP.process_batch; ``Fit`` calls it after each epoch when a validation_loader is given, prints
mAP@0.5 and mAP@0.5:0.95 and goes back to train(); without a loader the loop is the reference's.
"""
import torch

CLIP_NORM = 10.


def clip_gradient(model, clip_norm):
    """Scale every gradient by clip_norm / max(global L2 norm, clip_norm) (_fit.py:6-17).  Returns the norm."""
    grads = [p.grad for p in model.parameters() if p.requires_grad and p.grad is not None]
    if not grads:
        return 0.0
    total = torch.linalg.vector_norm(torch.stack(torch._foreach_norm(grads)).float()).item()     # sqrt(sum of squared norms), one read-back
    scale = clip_norm / max(total, clip_norm)
    if scale != 1.0:
        torch._foreach_mul_(grads, scale)
    return total


def _Train(model, train_loader, optimizer, log=print):
    model.train()
    for images, targets in train_loader:
        if torch.cuda.is_available():
            images, targets = images.cuda(non_blocking=True), targets.cuda(non_blocking=True)
        _, loss_rpn_cls, loss_rpn_box, loss_fast_cls, loss_fast_box = model(images, targets)
        optimizer.zero_grad()
        parts = torch.stack([l.reshape(()) for l in (loss_rpn_cls, loss_rpn_box, loss_fast_cls, loss_fast_box)])
        loss = parts.sum()
        loss.backward()
        if getattr(optimizer, 'clip_norm', None) is None:
            clip_gradient(model, CLIP_NORM)
        optimizer.step()
        if log:
            log(*torch.cat([loss.detach().reshape(1), parts.detach()]).tolist())


def targets_to_pixels(targets, height, width):
    """[T, 6] = image, class, normalised xywh (the training format) -> [T, 6] = image, class, xyxy in input pixels (what
    CalculateMAP.process_batch matches the detections against)."""
    from ..utils import xywh2xyxy
    scale = torch.tensor([width, height, width, height]).to(targets)
    return torch.cat([targets[:, :2], xywh2xyxy(targets[:, 2:6]) * scale], dim=1)


@torch.no_grad()
def Validate(model, validation_loader, args, metric=None):
    """mAP of a Faster R-CNN model over ``validation_loader`` (batches of images [B,3,H,W] and targets [T,6] = image, class, normalised
    xywh), entirely on the device: per batch one ``detect`` (input-pixel frame, thresholds args.inference_conf_thres /
    inference_iou_thres) and one matching launch (``metric.process_batch``); the rows are read back once, by ``metric.fetch()``, whose
    value -- (mAP per IoU threshold, mAP per class, class ids) -- is returned (zeros and no classes when nothing was detected or no
    target was seen).  The model is evaluated in eval() mode and put back into the mode it came in."""
    import numpy as np
    from ....metrics import CalculateMAP
    metric = CalculateMAP(np.linspace(0.5, 0.95, 10)) if metric is None else metric
    net = model.module if hasattr(model, 'module') else model
    was_training = net.training
    net.eval()
    try:
        for images, targets in validation_loader:
            images, targets = images.cuda(non_blocking=True), targets.cuda(non_blocking=True)
            dets, kept = net.detect(images, args.inference_conf_thres, args.inference_iou_thres)
            metric.process_batch(dets, kept, targets_to_pixels(targets.float(), images.size(2), images.size(3)))
    finally:
        net.train(was_training)
    metric.materialize()
    if not (metric.correct_all_images and metric.seen_all_targets_cls):
        return np.zeros(len(metric.map_iou_values)), np.zeros(0), []
    return metric.fetch()


def Fit(model, args, optimizer, train_loader, validation_loader=None):
    for epoch in range(args.start_epoch, args.total_epoch):
        if (epoch + 1) % 9 == 0:
            for group in optimizer.param_groups:
                group['lr'] = group['lr'] * 0.1
        print('\nEpoch {} learning_rate : {}'.format(epoch + 1, optimizer.param_groups[0]['lr']))
        _Train(model, train_loader, optimizer)
        state = (model.module if hasattr(model, 'module') else model).state_dict()
        torch.save(state, f'./{epoch + 1}.pth')
        if validation_loader is not None:
            map_each_iou = Validate(model, validation_loader, args)[0]
            print('Epoch {} mAP@0.5 : {:.4f}  mAP@0.5:0.95 : {:.4f}'.format(epoch + 1, float(map_each_iou[0]), float(map_each_iou.mean())))
            model.train()
