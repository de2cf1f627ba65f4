"""ResNeXt-50 32x4d / ResNeXt-101 32x8d on the MI355X kernels -- API mirror of the reference's classfication/models/resnext.py.

Same classes, constructor signatures, attribute names and ``state_dict()`` keys as the reference, and the same parameter construction
order.  The reference's quirks are kept: ``width_per_group`` doubles at the end of each ``_make_layer`` (conv2 is 128 / 256 / 512 / 1024
wide in resnext50_32x4d, twice that in resnext101_32x8d, always in 32 groups); ``Bottleneck`` takes its shortcut convolution whenever
``in_channels != 4 * mid_channels`` and puts the stride on ``conv2``; ``BasicBlock`` takes neither ``groups`` nor ``width_per_group``
(the reference's ``ResNet._make_layer`` passes both, so only ``Bottleneck`` can be built into a network there, and here);
``including_top=False`` returns ``[res5, res4, res3]``.  Unlike resnet.py this file calls NO ``initialize_weights``: the parameters keep
torch's default init, so ``torch.manual_seed`` reproduces the reference's.

``forward`` is the chain of resnet.py; the one new layer is conv2, a grouped 3x3 that ``resnet_ops.conv_bn_relu`` sends to
fva_gconv_fwd / fva_gconv_dgrad / fva_gconv_wgrad (csrc/grouped.hip).  Constructing a model needs no GPU; ``forward`` on CPU tensors raises.
"""
import torch.nn as nn

from ... import fc_ops, ops, resnet_ops
from .resnet import _tail

__all__ = ['ResNet', 'BasicBlock', 'Bottleneck', 'resnext50_32x4d', 'resnext101_32x8d']


def conv3x3(in_channels, out_channels, kernel_size=(3, 3), stride=(1, 1), padding=(1, 1), groups=1, bias=False):
    return nn.Conv2d(in_channels=in_channels, out_channels=out_channels, kernel_size=kernel_size, stride=stride, padding=padding, groups=groups,
                     bias=bias)


def conv1x1(in_channels, out_channels, kernel_size=(1, 1), stride=(1, 1), padding=(0, 0), bias=False):
    return nn.Conv2d(in_channels=in_channels, out_channels=out_channels, kernel_size=kernel_size, stride=stride, padding=padding, bias=bias)


def normalization(num_features):
    return nn.BatchNorm2d(num_features=num_features)


class Bottleneck(nn.Module):
    """1x1 to groups * width_per_group -> grouped 3x3 (carries the stride) -> 1x1 to 4 * mid, plus the shortcut (reference resnext.py:13-74)."""

    expansion = 4

    def __init__(self, in_channels, mid_channels, downsample=False, downsample_stride=(1, 1), groups=1, width_per_group=None):
        super().__init__()
        total_channels = groups * width_per_group
        self.down = downsample or in_channels != mid_channels * self.expansion
        self.conv1 = conv1x1(in_channels, total_channels)
        self.bn1 = normalization(total_channels)
        self.conv2 = conv3x3(total_channels, total_channels, stride=downsample_stride, groups=groups)
        self.bn2 = normalization(total_channels)
        self.conv3 = conv1x1(total_channels, mid_channels * self.expansion)
        self.bn3 = normalization(mid_channels * self.expansion)
        self.relu = nn.ReLU(inplace=True)
        if self.down:
            self.downsample = nn.Sequential(
                conv1x1(in_channels, mid_channels * self.expansion, stride=downsample_stride),
                normalization(mid_channels * self.expansion),
            )

    def forward(self, x):
        out = resnet_ops.conv_bn_relu(x, self.conv1, self.bn1)
        out = resnet_ops.conv_bn_relu(out, self.conv2, self.bn2)
        return _tail(self, out, self.conv3, self.bn3, x)


class BasicBlock(nn.Module):
    """3x3 (carries the stride) -> 3x3, plus the shortcut (reference resnext.py:76-127)."""

    expansion = 1

    def __init__(self, in_channels, mid_channels, downsample=False, downsample_stride=(1, 1)):
        super().__init__()
        self.down = downsample
        self.conv1 = conv3x3(in_channels, mid_channels, stride=downsample_stride)
        self.bn1 = normalization(mid_channels)
        self.conv2 = conv3x3(mid_channels, mid_channels * self.expansion)
        self.bn2 = normalization(mid_channels * self.expansion)
        self.relu = nn.ReLU(inplace=True)
        if self.down:
            self.downsample = nn.Sequential(
                conv1x1(in_channels, mid_channels * self.expansion, stride=downsample_stride),
                normalization(mid_channels * self.expansion),
            )

    def forward(self, x):
        out = resnet_ops.conv_bn_relu(x, self.conv1, self.bn1)
        return _tail(self, out, self.conv2, self.bn2, x)


class ResNet(nn.Module):
    """reference resnext.py:129-183.  ``including_top=False`` returns [res5, res4, res3].  No initialize_weights: torch's default init."""

    def __init__(self, in_channels, num_classes, num_blocks, basic_block, groups, width_per_group, including_top=True):
        super().__init__()
        self.including_top = including_top
        self.planes = 64
        self.groups = groups
        self.width_per_group = width_per_group
        self.conv1 = nn.Sequential(
            conv3x3(in_channels=in_channels, out_channels=self.planes, kernel_size=(7, 7), stride=(2, 2), padding=(3, 3)),
            normalization(self.planes),
            nn.ReLU(inplace=True),
        )
        self.pool1 = nn.Sequential(nn.MaxPool2d(kernel_size=(3, 3), stride=(2, 2), padding=(1, 1)))
        self.res2 = self._make_layer(basic_block, mid_channels=64, num_blocks=num_blocks[0])
        self.res3 = self._make_layer(basic_block, mid_channels=128, num_blocks=num_blocks[1], downsample=True, downsample_stride=(2, 2))
        self.res4 = self._make_layer(basic_block, mid_channels=256, num_blocks=num_blocks[2], downsample=True, downsample_stride=(2, 2))
        self.res5 = self._make_layer(basic_block, mid_channels=512, num_blocks=num_blocks[3], downsample=True, downsample_stride=(2, 2))
        if self.including_top:
            self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
            self.fc = nn.Linear(self.planes, num_classes)

    def _make_layer(self, basic_block, mid_channels, num_blocks, downsample=False, downsample_stride=(1, 1)):
        layers = [basic_block(in_channels=self.planes, mid_channels=mid_channels, downsample=downsample, downsample_stride=downsample_stride,
                              groups=self.groups, width_per_group=self.width_per_group)]
        self.planes = mid_channels * basic_block.expansion
        for _ in range(1, num_blocks):
            layers.append(basic_block(in_channels=self.planes, mid_channels=mid_channels, groups=self.groups, width_per_group=self.width_per_group))
        self.width_per_group *= 2                   # the reference's quirk: every stage's conv2 is twice as wide as the one before
        return nn.Sequential(*layers)

    def forward(self, x):
        if not x.is_cuda:
            raise RuntimeError('fastvision_amd ResNeXt: tensors must live on the GPU -- this package has no CPU path')
        x = resnet_ops.stem_bn_relu(x, self.conv1[0], self.conv1[1])
        x = resnet_ops.max_pool3s2(x)
        res2 = self.res2(x)
        res3 = self.res3(res2)
        res4 = self.res4(res3)
        res5 = self.res5(res4)
        if self.including_top:
            return fc_ops.linear(ops.global_avg_pool(res5), self.fc)
        return [res5, res4, res3]


def resnext101_32x8d(in_channels=3, num_classes=1000, including_top=True):
    return ResNet(in_channels=in_channels, num_classes=num_classes, num_blocks=[3, 4, 23, 3], basic_block=Bottleneck, groups=32, width_per_group=8,
                  including_top=including_top)


def resnext50_32x4d(in_channels=3, num_classes=1000, including_top=True):
    return ResNet(in_channels=in_channels, num_classes=num_classes, num_blocks=[3, 4, 6, 3], basic_block=Bottleneck, groups=32, width_per_group=4,
                  including_top=including_top)
