"""VGG classifiers on the MI355X kernels -- API mirror of the reference's classfication/models/vgg.py.

Same class, constructor signature, attribute names and ``state_dict()`` keys (``vgg1.0.weight``, ``vgg1.1.running_mean``,
``classifier.6.bias`` ...) and the same parameter construction order, so ``torch.manual_seed`` reproduces the reference's init and its
checkpoints load.  The ``nn.Conv2d`` / ``nn.BatchNorm2d`` / ``nn.ReLU`` / ``nn.Dropout`` / ``nn.Linear`` modules only own parameters and
settings; ``forward`` runs

    Conv2d -> ReLU                  vgg_ops.conv_bias_relu         (bias + ReLU in the convolution's epilogue)
    Conv2d -> BatchNorm2d -> ReLU   vgg_ops.conv_bn_relu           (``normal=True``: batch statistics, BatchNorm + ReLU passes)
    MaxPool2d(2, 2)                 vgg_ops.max_pool2
    AdaptiveAvgPool2d(7) + flatten  vgg_ops.adaptive_avg_pool7_flatten
    Linear -> ReLU -> Dropout       fc_ops.linear_relu, fc_ops.dropout
    Linear                          fc_ops.linear                  (fp32 logits [B, num_classes])

Dropout draws its masks on the device from ``_dropout_state`` (int64: seed, call counter), a NON-persistent buffer: it follows
``.to(device)``, is not part of ``state_dict()``, and is rolled back with the other buffers by ``graphs.snapshot_train_state``.  The seed
is ``torch.initial_seed()`` at construction -- ``torch.manual_seed(s)``, build, train gives the same bits every time -- and both Dropout
layers share the one state (every call advances the counter on the device, so a captured train step draws new masks on every replay).
``nn.Dropout.p`` and ``.training`` are read at call time.  Constructing a model needs no GPU; ``forward`` on CPU tensors raises.
"""
import torch
import torch.nn as nn

from ... import fc_ops, vgg_ops

__all__ = ['VGG', 'vgg11', 'vgg11_bn', 'vgg13', 'vgg13_bn', 'vgg16', 'vgg16_bn', 'vgg19', 'vgg19_bn']


def conv3x3(in_channels, out_channels, kernel_size=(3, 3), stride=(1, 1), padding=(1, 1), groups=1, bias=False):
    return nn.Conv2d(in_channels=in_channels, out_channels=out_channels, kernel_size=kernel_size, stride=stride, padding=padding, groups=groups, bias=bias)


def normalization(num_features):
    return nn.BatchNorm2d(num_features=num_features)


class VGG(nn.Module):
    def __init__(self, in_channels, num_classes, num_blocks, channels, normal=False):
        super().__init__()
        self.in_channles = in_channels          # (sic: the reference's attribute name)
        self.normal = normal
        self.vgg1 = self._make_layer(num_blocks[0], channels[0])
        self.vgg2 = self._make_layer(num_blocks[1], channels[1])
        self.vgg3 = self._make_layer(num_blocks[2], channels[2])
        self.vgg4 = self._make_layer(num_blocks[3], channels[3])
        self.vgg5 = self._make_layer(num_blocks[4], channels[4])
        self.maxpool = nn.MaxPool2d(kernel_size=(2, 2), stride=2)
        self.gmp = nn.AdaptiveAvgPool2d((7, 7))
        self.classifier = nn.Sequential(nn.Linear(channels[3] * 7 * 7, 4096), nn.ReLU(True), nn.Dropout(), nn.Linear(4096, 4096), nn.ReLU(True),
                                        nn.Dropout(), nn.Linear(4096, num_classes))
        self.register_buffer('_dropout_state', fc_ops.new_dropout_state(), persistent=False)

    def _make_layer(self, num_blocks, channels):
        layers = []
        for _ in range(num_blocks):
            layers.append(conv3x3(in_channels=self.in_channles, out_channels=channels, bias=True))
            if self.normal:
                layers.append(normalization(channels))
            layers.append(nn.ReLU(inplace=True))
            self.in_channles = channels
        return nn.Sequential(*layers)

    @staticmethod
    def _stage(x, seq):
        layers = list(seq)
        for i, layer in enumerate(layers):
            if isinstance(layer, nn.Conv2d):          # the BatchNorm2d / ReLU that follow it in the Sequential are fused into this call
                nxt = layers[i + 1] if i + 1 < len(layers) else None
                x = vgg_ops.conv_bn_relu(x, layer, nxt) if isinstance(nxt, nn.BatchNorm2d) else vgg_ops.conv_bias_relu(x, layer)
        return x

    def forward(self, x):
        if not x.is_cuda:
            raise RuntimeError('fastvision_amd VGG: tensors must live on the GPU -- this package has no CPU path')
        for stage in (self.vgg1, self.vgg2, self.vgg3, self.vgg4, self.vgg5):
            x = vgg_ops.max_pool2(self._stage(x, stage))
        x = vgg_ops.adaptive_avg_pool7_flatten(x)
        c = self.classifier
        x = fc_ops.dropout(fc_ops.linear_relu(x, c[0]), c[2], self._dropout_state)
        x = fc_ops.dropout(fc_ops.linear_relu(x, c[3]), c[5], self._dropout_state)
        return fc_ops.linear(x, c[6])


_WIDTHS = [64, 128, 256, 512, 512]


def vgg11(in_channels=3, num_classes=1000):
    return VGG(in_channels=in_channels, num_classes=num_classes, num_blocks=[1, 1, 2, 2, 2], channels=list(_WIDTHS))


def vgg11_bn(in_channels=3, num_classes=1000):
    return VGG(in_channels=in_channels, num_classes=num_classes, num_blocks=[1, 1, 2, 2, 2], channels=list(_WIDTHS), normal=True)


def vgg13(in_channels=3, num_classes=1000):
    return VGG(in_channels=in_channels, num_classes=num_classes, num_blocks=[2, 2, 2, 2, 2], channels=list(_WIDTHS))


def vgg13_bn(in_channels=3, num_classes=1000):
    return VGG(in_channels=in_channels, num_classes=num_classes, num_blocks=[2, 2, 2, 2, 2], channels=list(_WIDTHS), normal=True)


def vgg16(in_channels=3, num_classes=1000):
    return VGG(in_channels=in_channels, num_classes=num_classes, num_blocks=[2, 2, 3, 3, 3], channels=list(_WIDTHS))


def vgg16_bn(in_channels=3, num_classes=1000):
    return VGG(in_channels=in_channels, num_classes=num_classes, num_blocks=[2, 2, 3, 3, 3], channels=list(_WIDTHS), normal=True)


def vgg19(in_channels=3, num_classes=1000):
    return VGG(in_channels=in_channels, num_classes=num_classes, num_blocks=[2, 2, 4, 4, 4], channels=list(_WIDTHS))


def vgg19_bn(in_channels=3, num_classes=1000):
    return VGG(in_channels=in_channels, num_classes=num_classes, num_blocks=[2, 2, 4, 4, 4], channels=list(_WIDTHS), normal=True)
