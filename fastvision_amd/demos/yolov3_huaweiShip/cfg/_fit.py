"""Fit loop of the ship demo -- API mirror of the reference's demos/yolov3_huaweiShip/cfg/_fit.py (Fit, _Train).

Epoch contract (_fit.py:12-32): the last ``no_aug_epoch`` epochs train on the validation loader (no augmentation); a ``best-epoch_*``
checkpoint on a better mean train loss and an ``epoch_*`` checkpoint every epoch; ``scheduler.step()`` only for
``warmup_epoch <= epoch < total_epoch - no_aug_epoch - 1``.  Step contract (:40-69): while ``epoch < warmup_epoch`` every group's
learning rate is the linear ramp from ``warmup_init_lr`` to ``init_lr`` over ``warmup_iters`` iterations, in the no-augmentation phase
it is ``min_lr``; predict = model(images); optimizer.zero_grad(); the three losses, their sum, backward, step.  The loss is read back
once per batch (the reference reads it twice), for the log line and the epoch mean.
"""
import time

import torch

_BATCH_LINE = 'epoch : {} batch : {} / {} loss : {:.3f} lr : {:.8f} time : {:.3f}'


def _set_lr(optimizer, lr):
    for group in optimizer.param_groups:
        group['lr'] = lr


def _Train(model, train_loader, optimizer, criterion, epoch, args, log=print):
    model.train()
    batches = len(train_loader)
    total = 0.0
    for batch, (images, target) in enumerate(train_loader):
        tick = time.time()
        if epoch < args.warmup_epoch:
            it = epoch * batches + batch
            _set_lr(optimizer, (args.init_lr - args.warmup_init_lr) * it / float(args.warmup_iters) + args.warmup_init_lr)
        if epoch >= args.total_epoch - args.no_aug_epoch:
            _set_lr(optimizer, args.min_lr)
        if torch.cuda.is_available():
            images, target = images.cuda(non_blocking=True), target.cuda(non_blocking=True)
        predict = model(images)
        optimizer.zero_grad()
        loss_box, loss_cls, loss_conf = criterion(predict, target, model)
        loss = loss_box + loss_cls + loss_conf
        loss.backward()
        optimizer.step()
        value = loss.item()
        total += value
        if log:
            log(_BATCH_LINE.format(str(epoch + 1).rjust(3, '0'), batch + 1, batches, value, optimizer.param_groups[0]['lr'], time.time() - tick))
    return total / batches


def Fit(model, args, optimizer, criterion, metric, scheduler, train_loader, validation_loader):
    best = float('inf')
    for epoch in range(args.start_epoch, args.total_epoch):
        started = time.time()
        print('\nEpoch {} learning_rate : {}'.format(epoch + 1, optimizer.param_groups[0]['lr']))
        no_aug = epoch >= args.total_epoch - args.no_aug_epoch
        if no_aug:
            print('using validation_loader for no_aug')
        loss_train = _Train(model, validation_loader if no_aug else train_loader, optimizer, criterion, epoch, args)
        state = (model.module if hasattr(model, 'module') else model).state_dict()
        tag = str(epoch + 1).rjust(3, '0')
        if loss_train < best:
            torch.save(state, f'./best-epoch_{tag}_loss_{loss_train}.pth')
            best = loss_train
        torch.save(state, f'./epoch_{tag}_loss_{loss_train}.pth')
        print('epoch : {} train_loss : {:.3f} time : {:.3f}'.format(tag, loss_train, time.time() - started))
        if args.warmup_epoch <= epoch < args.total_epoch - args.no_aug_epoch - 1:
            scheduler.step()
