"""ResNeXt restated in plain torch: the CPU side of tests/test_resnext_restatement_cpu.py, tests/test_gpu_grouped.py and
tests/test_gpu_resnext.py.  Not a test module (pytest does not collect it).

    gconv_reference         the grouped 3x3 convolution (padding 1, stride 1 or 2) in ``dt``: y, dx, dw and the per-channel sums of y and y^2,
                            written with explicit shifted slices (the CPU test pins it against F.conv2d(..., groups=) and autograd), and the
                            magnitudes the limits of tests/streaming_measure.py need
    StockResNeXt            resnext50_32x4d / resnext101_32x8d from stock torch.nn modules, layer for layer what the reference's
                            classfication/models/resnext.py builds: default init (no initialize_weights), width_per_group doubling per stage
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from resnet_restatement import StockResNet

NAMES = ['resnext50_32x4d', 'resnext101_32x8d']
BLOCKS = {'resnext50_32x4d': ([3, 4, 6, 3], 32, 4), 'resnext101_32x8d': ([3, 4, 23, 3], 32, 8)}


# ------------------------------------------------------------------------------------------------ the grouped convolution
def _taps(xp, kh, kw, OH, OW, s):
    """xp [B, H+2, W+2, ...] zero-padded by one: the pixels tap (kh, kw) of every output pixel reads"""
    return xp[:, kh:kh + s * (OH - 1) + 1:s, kw:kw + s * (OW - 1) + 1:s]


def gconv_reference(x, w, dy, groups, stride, dt):
    """x [B, H, W, C] and dy [B, OH, OW, C] channels-last, w [C, Cg, 3, 3]; everything evaluated in ``dt`` from the operands as given.
    Returns a dict: y [B, OH, OW, C], dx [B, H, W, C], dw [C, Cg, 3, 3], s1 / s2 [C] (sums of y and y^2 over the pixels), and for each of
    y, dx, dw the largest |term| of the element's sum (``*_mag``) and for the sums the sums of |y| and y^2 (``s1_abs``, ``s2_abs``)."""
    B, H, W, Cc = x.shape
    Cg, s = Cc // groups, stride
    OH, OW = (H - 1) // s + 1, (W - 1) // s + 1
    x, w, dy = x.to(dt), w.to(dt), dy.to(dt)
    xp = torch.zeros(B, H + 2, W + 2, groups, Cg, dtype=dt)
    xp[:, 1:1 + H, 1:1 + W] = x.view(B, H, W, groups, Cg)
    wg = w.view(groups, Cg, Cg, 3, 3)                       # [g][co][ci][kh][kw]
    dyg = dy.view(B, OH, OW, groups, Cg)
    y = torch.zeros(B, OH, OW, groups, Cg, dtype=dt)
    y_mag = torch.zeros_like(y)
    dxp = torch.zeros_like(xp)
    dxp_mag = torch.zeros_like(xp)
    dw = torch.zeros(groups, Cg, Cg, 3, 3, dtype=dt)
    dw_mag = torch.zeros_like(dw)
    for kh in range(3):
        for kw in range(3):
            t = _taps(xp, kh, kw, OH, OW, s)                 # [B, OH, OW, g, ci]
            wk = wg[:, :, :, kh, kw]                         # [g, co, ci]
            y += torch.einsum('bhwgi,goi->bhwgo', t, wk)
            y_mag = torch.maximum(y_mag, torch.einsum('bhwgi,goi->bhwgoi', t.abs(), wk.abs()).amax(-1))
            d = _taps(dxp, kh, kw, OH, OW, s)
            d += torch.einsum('bhwgo,goi->bhwgi', dyg, wk)
            m = _taps(dxp_mag, kh, kw, OH, OW, s)
            m.copy_(torch.maximum(m, torch.einsum('bhwgo,goi->bhwgio', dyg.abs(), wk.abs()).amax(-1)))
            dw[:, :, :, kh, kw] = torch.einsum('bhwgo,bhwgi->goi', dyg, t)
            dw_mag[:, :, :, kh, kw] = (dyg.abs().unsqueeze(-1) * t.abs().unsqueeze(-2)).amax((0, 1, 2))
    y = y.view(B, OH, OW, Cc)
    return {'y': y, 'y_mag': y_mag.view(B, OH, OW, Cc),
            'dx': dxp[:, 1:1 + H, 1:1 + W].reshape(B, H, W, Cc), 'dx_mag': dxp_mag[:, 1:1 + H, 1:1 + W].reshape(B, H, W, Cc),
            'dw': dw.view(Cc, Cg, 3, 3), 'dw_mag': dw_mag.view(Cc, Cg, 3, 3),
            's1': y.sum((0, 1, 2)), 's2': (y * y).sum((0, 1, 2)), 's1_abs': y.abs().sum((0, 1, 2)), 's2_abs': (y * y).sum((0, 1, 2))}


# ------------------------------------------------------------------------------------------------ the classifiers from stock modules
def _conv(cin, cout, k, stride=1, groups=1):
    return nn.Conv2d(cin, cout, kernel_size=(k, k), stride=(stride, stride), padding=(k // 2, k // 2), groups=groups, bias=False)


class _XBlock(nn.Module):
    """The ResNeXt bottleneck: 1x1 to groups * width, grouped 3x3 with the stride, 1x1 to 4 * mid; a shortcut convolution whenever the
    widths differ, also at stride 1.  Modules in the reference's construction order."""

    kind = 'bottleneck'

    def __init__(self, cin, mid, down, stride, groups, width):
        super().__init__()
        total, cout = groups * width, mid * 4
        self.down = down or cin != cout
        self.conv1, self.bn1 = _conv(cin, total, 1), nn.BatchNorm2d(total)
        self.conv2, self.bn2 = _conv(total, total, 3, stride, groups), nn.BatchNorm2d(total)
        self.conv3, self.bn3 = _conv(total, cout, 1), nn.BatchNorm2d(cout)
        self.relu = nn.ReLU(inplace=True)
        if self.down:
            self.downsample = nn.Sequential(_conv(cin, cout, 1, stride), nn.BatchNorm2d(cout))

    def units(self):
        return [(self.conv1, self.bn1), (self.conv2, self.bn2), (self.conv3, self.bn3)]


class StockResNeXt(StockResNet):
    """StockResNet's hooks (``act``, ``pool``, ``store``, ``wround``) and chain; ``run`` passes the convolution's groups.  Default init."""

    def __init__(self, name, in_channels=3, num_classes=1000, including_top=True):
        nn.Module.__init__(self)
        blocks, groups, width = BLOCKS[name]
        self.including_top = including_top
        self.conv1 = nn.Sequential(_conv(in_channels, 64, 7, 2), nn.BatchNorm2d(64), nn.ReLU(inplace=True))
        self.pool1 = nn.Sequential(nn.MaxPool2d(kernel_size=(3, 3), stride=(2, 2), padding=(1, 1)))
        planes = 64
        for stage, (n, mid) in enumerate(zip(blocks, (64, 128, 256, 512)), start=2):
            first = stage > 2
            layers = [_XBlock(planes, mid, first, 2 if first else 1, groups, width)]
            planes = mid * 4
            layers += [_XBlock(planes, mid, False, 1, groups, width) for _ in range(1, n)]
            width *= 2
            setattr(self, f'res{stage}', nn.Sequential(*layers))
        if including_top:
            self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
            self.fc = nn.Linear(planes, num_classes)

    def forward(self, x, act=None, pool=None, store=None, wround=None):
        act = act or (lambda u, info: F.relu(u))
        pool = pool or (lambda t: F.max_pool2d(t, 3, 2, 1))
        store = store or (lambda t: t)
        wround = wround or (lambda w: w)

        def run(conv, t):
            return store(F.conv2d(t, wround(conv.weight), None, conv.stride, conv.padding, 1, conv.groups))

        conv, bn = self.conv1[0], self.conv1[1]
        x = store(x)
        y = run(conv, x)
        x = store(act(bn(y), {'name': 'conv1', 'x': x, 'conv': conv, 'bn': bn, 'y': y, 'short': None}))
        x = pool(x)
        taps = []
        for stage in (2, 3, 4, 5):
            for i, blk in enumerate(getattr(self, f'res{stage}')):
                inp, units = x, blk.units()
                for j, (conv, bn) in enumerate(units):
                    y = run(conv, x)
                    u, short = bn(y), None
                    if j == len(units) - 1:
                        if blk.down:
                            cd, bd = blk.downsample[0], blk.downsample[1]
                            yd = run(cd, inp)
                            u, short = u + bd(yd), ('conv', inp, cd, bd, yd)
                        else:
                            u, short = u + inp, ('identity', inp)
                    x = store(act(u, {'name': f'res{stage}.{i}.{j}', 'x': x, 'conv': conv, 'bn': bn, 'y': y, 'short': short}))
            taps.append(x)
        if self.including_top:
            return F.linear(store(torch.flatten(self.avgpool(x), 1)), wround(self.fc.weight), self.fc.bias)
        return [taps[3], taps[2], taps[1]]
