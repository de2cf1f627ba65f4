"""Frozen BatchNorm for fine-tuning: the BatchNorm2d modules stay in eval mode (running statistics fixed, never updated) while the
convolutions and the affine parameters keep training -- the usual way to stop a small fine-tuning batch from overwriting pretrained
statistics.  ``model.train()`` (which ``Fit._train`` calls every epoch) puts every submodule back into training mode, so a plain
``bn.eval()`` does not survive it; ``freeze_batchnorm`` makes the mode stick.

The module object stays what it was: only its class is exchanged for a subclass whose ``train()`` ignores the requested mode, so the
state_dict keys, the parameter objects (what the optimizer holds) and the buffer objects do not change, and the module still pickles
and deep-copies (the subclass lives at module level)."""
import torch.nn as nn

__all__ = ['freeze_batchnorm', 'unfreeze_batchnorm', 'FrozenBatchNorm2d']


class FrozenBatchNorm2d(nn.BatchNorm2d):
    """nn.BatchNorm2d whose ``training`` flag stays False through ``.train()`` calls."""

    def train(self, mode=True):
        return super().train(False)


def freeze_batchnorm(module):
    """Put every ``nn.BatchNorm2d`` under ``module`` (itself included) into eval mode and keep it there through later ``.train()``
    calls.  Returns ``module``."""
    for m in module.modules():
        if type(m) is FrozenBatchNorm2d:
            continue
        if isinstance(m, nn.BatchNorm2d):
            if type(m) is not nn.BatchNorm2d:
                raise TypeError(f'freeze_batchnorm: {type(m).__name__} is a subclass of nn.BatchNorm2d with behaviour of its own; '
                                'only plain nn.BatchNorm2d modules are frozen')
            m.__class__ = FrozenBatchNorm2d
            m.training = False
    return module


def unfreeze_batchnorm(module):
    """Undo ``freeze_batchnorm``: every frozen BatchNorm under ``module`` is a plain ``nn.BatchNorm2d`` again, in the mode of the module
    that holds it.  Returns ``module``."""
    def visit(m, mode):
        if type(m) is FrozenBatchNorm2d:
            m.__class__ = nn.BatchNorm2d
            m.training = mode
        for child in m.children():
            visit(child, m.training)
    visit(module, module.training)
    return module
