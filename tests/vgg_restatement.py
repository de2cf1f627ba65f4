"""The VGG classifiers restated from stock ``torch.nn`` modules: the CPU side of tests/test_vgg_cpu.py and tests/test_gpu_vgg_classify.py.
Not a test module (pytest does not collect it).  Layer for layer what the reference's classfication/models/vgg.py builds: five stages of
``Conv2d(3x3, padding 1, bias) [-> BatchNorm2d] -> ReLU``, ``MaxPool2d(2, 2)`` after each, ``AdaptiveAvgPool2d((7, 7))``, flatten,
``Linear -> ReLU -> Dropout -> Linear -> ReLU -> Dropout -> Linear``."""
import numpy as np
import torch
import torch.nn as nn

BLOCKS = {'vgg11': [1, 1, 2, 2, 2], 'vgg13': [2, 2, 2, 2, 2], 'vgg16': [2, 2, 3, 3, 3], 'vgg19': [2, 2, 4, 4, 4]}
WIDTHS = [64, 128, 256, 512, 512]
NAMES = ['vgg11', 'vgg11_bn', 'vgg13', 'vgg13_bn', 'vgg16', 'vgg16_bn', 'vgg19', 'vgg19_bn']


class StockVGG(nn.Module):
    def __init__(self, name, in_channels=3, num_classes=1000):
        super().__init__()
        bn = name.endswith('_bn')
        width = in_channels
        for stage, (blocks, out) in enumerate(zip(BLOCKS[name.replace('_bn', '')], WIDTHS), start=1):
            layers = []
            for _ in range(blocks):
                layers.append(nn.Conv2d(width, out, kernel_size=3, stride=1, padding=1, bias=True))
                if bn:
                    layers.append(nn.BatchNorm2d(out))
                layers.append(nn.ReLU(inplace=True))
                width = out
            setattr(self, f'vgg{stage}', nn.Sequential(*layers))
        self.maxpool = nn.MaxPool2d(kernel_size=(2, 2), stride=2)
        self.gmp = nn.AdaptiveAvgPool2d((7, 7))
        self.classifier = nn.Sequential(nn.Linear(WIDTHS[3] * 49, 4096), nn.ReLU(True), nn.Dropout(), nn.Linear(4096, 4096), nn.ReLU(True),
                                        nn.Dropout(), nn.Linear(4096, num_classes))

    def forward(self, x):
        for stage in (self.vgg1, self.vgg2, self.vgg3, self.vgg4, self.vgg5):
            x = self.maxpool(stage(x))
        return self.classifier(torch.flatten(self.gmp(x), 1))


def set_dropout(model, p):
    for m in model.modules():
        if isinstance(m, nn.Dropout):
            m.p = p


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox-4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11) on numpy uint64 arrays holding 32-bit words: the ten rounds as published.
    tests/test_vgg_cpu.py pins this restatement to the known-answer vectors of the Random123 distribution; the GPU test compares the
    device's dropout masks with it."""
    m32 = np.uint64(0xFFFFFFFF)
    c = [np.asarray(v, dtype=np.uint64) & m32 for v in (c0, c1, c2, c3)]
    k = [np.uint64(k0) & m32, np.uint64(k1) & m32]
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & m32]
        k = [(k[0] + np.uint64(0x9E3779B9)) & m32, (k[1] + np.uint64(0xBB67AE85)) & m32]
    return c


def dropout_keep_mask(seed, counter, n, p):
    """The keep mask of n elements as include/fastvision_amd.h defines it: element e takes word e % 4 of
    philox(counter = (e / 4, 0, call counter lo, hi), key = (seed lo, hi)); keep = word >= p * 2^32."""
    groups = np.arange((n + 3) // 4, dtype=np.uint64)
    zero = np.zeros_like(groups)
    w = philox4x32_10(groups, zero, zero + np.uint64(counter & 0xFFFFFFFF), zero + np.uint64(counter >> 32), seed & 0xFFFFFFFF, seed >> 32)
    words = np.stack(w, axis=1).reshape(-1)[:n]
    p = float(np.float32(p))                      # the C ABI takes p as a float
    return torch.from_numpy(words >= np.uint64(min(int(p * 4294967296.0), 4294967295)))
