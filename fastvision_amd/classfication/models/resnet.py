"""ResNet-18 / 34 / 50 / 101 / 152 on the MI355X kernels -- API mirror of the reference's classfication/models/resnet.py.

Same classes, constructor signatures, attribute names and ``state_dict()`` keys (``conv1.0.weight``, ``res2.0.downsample.1.running_var``,
``fc.bias`` ...), the same parameter construction order and the same ``initialize_weights`` at the end of ``ResNet.__init__``, so
``torch.manual_seed`` reproduces the reference's init and its checkpoints load strictly.  The reference's quirks are kept: ``Bottleneck``
takes its shortcut convolution whenever ``in_channels != 4 * mid_channels`` (a stride-1 64 -> 256 shortcut in ``res2.0``) and puts the
stride on ``conv2``; ``BasicBlock`` puts it on ``conv1``; ``including_top=False`` returns ``[res5, res4, res3]``.

The ``nn`` modules only own parameters and settings; ``forward`` runs

    conv1 (7x7 s2) -> BN -> ReLU       resnet_ops.stem_bn_relu        (patch matrix + 1x1 implicit GEMM)
    MaxPool2d(3, 2, 1)                 resnet_ops.max_pool3s2
    conv -> BN -> ReLU                 resnet_ops.conv_bn_relu
    conv -> BN -> (+ shortcut) -> ReLU resnet_ops.conv_bn_add_relu    (the add inside the ReLU; identity or 1x1 shortcut of stride 1 / 2)
    AdaptiveAvgPool2d(1) + flatten     ops.global_avg_pool
    Linear                             fc_ops.linear                  (fp32 logits [B, num_classes])

Constructing a model needs no GPU; ``forward`` on CPU tensors raises.  ResNeXt lives in resnext.py: this chain with a
grouped conv2 (csrc/grouped.hip).
"""
import torch.nn as nn

from ... import fc_ops, ops, resnet_ops

__all__ = ['ResNet', 'BasicBlock', 'Bottleneck', 'resnet18', 'resnet34', 'resnet50', 'resnet101', 'resnet152']


def conv3x3(in_channels, out_channels, kernel_size=(3, 3), stride=(1, 1), padding=(1, 1), bias=False):
    return nn.Conv2d(in_channels=in_channels, out_channels=out_channels, kernel_size=kernel_size, stride=stride, padding=padding, bias=bias)


def conv1x1(in_channels, out_channels, kernel_size=(1, 1), stride=(1, 1), padding=(0, 0), bias=False):
    return nn.Conv2d(in_channels=in_channels, out_channels=out_channels, kernel_size=kernel_size, stride=stride, padding=padding, bias=bias)


def normalization(num_features):
    return nn.BatchNorm2d(num_features=num_features)


def initialize_weights(model):
    """utils.initialize_weights of the reference, for the module types a ResNet holds (same order, same draws)."""
    for m in model.modules():
        if isinstance(m, nn.Conv2d):
            nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.BatchNorm2d):
            nn.init.constant_(m.weight, 1)
            nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.Linear):
            nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
            nn.init.constant_(m.bias, 0)


def _tail(block, x, conv, bn, identity):
    if block.down:
        return resnet_ops.conv_bn_add_relu(x, conv, bn, identity, block.downsample[0], block.downsample[1])
    return resnet_ops.conv_bn_add_relu(x, conv, bn, identity)


class Bottleneck(nn.Module):
    """1x1 -> 3x3 (carries the stride) -> 1x1 to 4 * mid, plus the shortcut (reference resnet.py:14-73)."""

    expansion = 4

    def __init__(self, in_channels, mid_channels, downsample=False, downsample_stride=(1, 1)):
        super().__init__()
        self.down = downsample or in_channels != mid_channels * self.expansion
        self.conv1 = conv1x1(in_channels, mid_channels)
        self.bn1 = normalization(mid_channels)
        self.conv2 = conv3x3(mid_channels, mid_channels, stride=downsample_stride)
        self.bn2 = normalization(mid_channels)
        self.conv3 = conv1x1(mid_channels, mid_channels * self.expansion)
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
    """3x3 (carries the stride) -> 3x3, plus the shortcut (reference resnet.py:75-126)."""

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
    """reference resnet.py:128-181.  ``including_top=False`` returns [res5, res4, res3]."""

    def __init__(self, in_channels, num_classes, num_blocks, basic_block, including_top=True):
        super().__init__()
        self.including_top = including_top
        self.planes = 64
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
        initialize_weights(self)

    def _make_layer(self, basic_block, mid_channels, num_blocks, downsample=False, downsample_stride=(1, 1)):
        layers = [basic_block(in_channels=self.planes, mid_channels=mid_channels, downsample=downsample, downsample_stride=downsample_stride)]
        self.planes = mid_channels * basic_block.expansion
        for _ in range(1, num_blocks):
            layers.append(basic_block(in_channels=self.planes, mid_channels=mid_channels))
        return nn.Sequential(*layers)

    def forward(self, x):
        if not x.is_cuda:
            raise RuntimeError('fastvision_amd ResNet: tensors must live on the GPU -- this package has no CPU path')
        x = resnet_ops.stem_bn_relu(x, self.conv1[0], self.conv1[1])
        x = resnet_ops.max_pool3s2(x)
        res2 = self.res2(x)
        res3 = self.res3(res2)
        res4 = self.res4(res3)
        res5 = self.res5(res4)
        if self.including_top:      # fva_gap_fwd on the halo view of res5, then the biased fc GEMM (fp32 logits)
            return fc_ops.linear(ops.global_avg_pool(res5), self.fc)
        return [res5, res4, res3]


def resnet18(in_channels=3, num_classes=1000, including_top=True):
    return ResNet(in_channels=in_channels, num_classes=num_classes, num_blocks=[2, 2, 2, 2], basic_block=BasicBlock, including_top=including_top)


def resnet34(in_channels=3, num_classes=1000, including_top=True):
    return ResNet(in_channels=in_channels, num_classes=num_classes, num_blocks=[3, 4, 6, 3], basic_block=BasicBlock, including_top=including_top)


def resnet50(in_channels=3, num_classes=1000, including_top=True):
    return ResNet(in_channels=in_channels, num_classes=num_classes, num_blocks=[3, 4, 6, 3], basic_block=Bottleneck, including_top=including_top)


def resnet101(in_channels=3, num_classes=1000, including_top=True):
    return ResNet(in_channels=in_channels, num_classes=num_classes, num_blocks=[3, 4, 23, 3], basic_block=Bottleneck, including_top=including_top)


def resnet152(in_channels=3, num_classes=1000, including_top=True):
    return ResNet(in_channels=in_channels, num_classes=num_classes, num_blocks=[3, 8, 36, 3], basic_block=Bottleneck, including_top=including_top)
