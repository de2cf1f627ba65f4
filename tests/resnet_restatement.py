"""The ResNet pieces restated in plain torch: the CPU side of tests/test_resnet_restatement_cpu.py, tests/test_gpu_resnet_kernels.py and
tests/test_gpu_resnet.py.  Not a test module (pytest does not collect it).  Every formula takes ``dt``: torch.float64 is the reference,
torch.float32 the honest fp32 evaluation whose distance from it feeds the limits of tests/streaming_measure.py.

    patch_matrix            the 7x7 / stride 2 / pad 3 stem as a matrix [B*OH*OW][Kp], column ci*49 + kh*7 + kw (include/fastvision_amd.h)
    maxpool3s2 / _bwd       MaxPool2d(3, 2, 1) over NHWC with torch's scan (the first maximum wins, a NaN wins over everything)
    subsample2 / _bwd       x[:, ::2, ::2] and its scatter back with zeros
    add_relu_*              z = relu(bn(y) + R), R the identity or a second normalised tensor, its backward sums and dY
    StockResNet             the five classifiers from stock torch.nn modules, layer for layer what classfication/models/resnet.py builds
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

NAMES = ['resnet18', 'resnet34', 'resnet50', 'resnet101', 'resnet152']
BLOCKS = {'resnet18': ('basic', [2, 2, 2, 2]), 'resnet34': ('basic', [3, 4, 6, 3]), 'resnet50': ('bottleneck', [3, 4, 6, 3]),
          'resnet101': ('bottleneck', [3, 4, 23, 3]), 'resnet152': ('bottleneck', [3, 8, 36, 3])}


# ------------------------------------------------------------------------------------------------ the stem's patch matrix
def stem_kp(cin, bf16):
    """Cin * 49 rounded up to a whole 128-byte k-tile of the implicit GEMM: 32 columns in fp32, 64 in bf16."""
    bk = 64 if bf16 else 32
    return (cin * 49 + bk - 1) // bk * bk


def patch_matrix(x, kp):
    """x [B, Cin, H, W] -> P [B*OH*OW, kp]: column ci*49 + kh*7 + kw = x[b, ci, 2 oy - 3 + kh, 2 ox - 3 + kw], zero outside the image and
    from column Cin*49 on.  Written with explicit indices, not unfold (the CPU test pins it against F.unfold)."""
    B, Cin, H, W = x.shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = torch.zeros(B, Cin, H + 6, W + 6, dtype=x.dtype)
    xp[:, :, 3:3 + H, 3:3 + W] = x
    P = torch.zeros(B, OH, OW, kp, dtype=x.dtype)
    for ci in range(Cin):
        for kh in range(7):
            for kw in range(7):
                P[:, :, :, ci * 49 + kh * 7 + kw] = xp[:, ci, kh:kh + 2 * OH:2, kw:kw + 2 * OW:2][:, :OH, :OW]
    return P.reshape(B * OH * OW, kp)


# ------------------------------------------------------------------------------------------------ MaxPool2d(3, 2, 1), NHWC
def _windows3(x):
    """x [B, H, W, C] -> (taps [B, OH, OW, 9, C] in scan order kh, kw; valid [OH, OW, 9]): taps outside the image are marked invalid"""
    B, H, W, Cc = x.shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = torch.zeros(B, 2 * OH + 1, 2 * OW + 1, Cc, dtype=x.dtype)
    ok = torch.zeros(2 * OH + 1, 2 * OW + 1, dtype=torch.bool)
    xp[:, 1:1 + H, 1:1 + W] = x
    ok[1:1 + H, 1:1 + W] = True
    taps, valid = [], []
    for kh in range(3):
        for kw in range(3):
            taps.append(xp[:, kh:kh + 2 * OH:2, kw:kw + 2 * OW:2][:, :OH, :OW])
            valid.append(ok[kh:kh + 2 * OH:2, kw:kw + 2 * OW:2][:OH, :OW])
    return torch.stack(taps, 3), torch.stack(valid, 2)


def maxpool3s2_argmax(x):
    """The tap (0..8) on which torch's scan ``if v > m or isnan(v): m, arg = v, tap`` ends, from m = -inf over the valid taps: the FIRST
    maximum of a window, or its LAST NaN.  x [B, H, W, C] -> arg [B, OH, OW, C]."""
    taps, valid = _windows3(x)
    v = valid[None, :, :, :, None]
    t = torch.where(v, taps, torch.full_like(taps, float('-inf')))
    idx = torch.arange(9).view(1, 1, 1, 9, 1).expand_as(t)
    nan = torch.isnan(t)
    clean = torch.where(nan, torch.full_like(t, float('-inf')), t)
    m = clean.max(3, keepdim=True).values
    first = torch.where((clean == m) & v & ~nan, idx, torch.full_like(idx, 9)).min(3).values
    last_nan = torch.where(nan, idx, torch.full_like(idx, -1)).max(3).values
    return torch.where(last_nan >= 0, last_nan, first)


def maxpool3s2(x):
    """x [B, H, W, C] -> (out [B, OH, OW, C], arg): out is the selected tap itself (a copy, bit for bit)"""
    taps, _ = _windows3(x)
    arg = maxpool3s2_argmax(x)
    return taps.gather(3, arg.unsqueeze(3)).squeeze(3), arg


def maxpool3s2_bwd(dz, x):
    """dz [B, OH, OW, C], x [B, H, W, C] -> dx [B, H, W, C]: every dz lands on the one pixel its window selected, overlapping windows add"""
    B, H, W, Cc = x.shape
    OH, OW = dz.shape[1], dz.shape[2]
    arg = maxpool3s2_argmax(x)
    dxp = torch.zeros(B, 2 * OH + 1, 2 * OW + 1, Cc, dtype=dz.dtype)
    for kh in range(3):
        for kw in range(3):
            dxp[:, kh:kh + 2 * OH:2, kw:kw + 2 * OW:2][:, :OH, :OW] += torch.where(arg == kh * 3 + kw, dz, torch.zeros_like(dz))
    return dxp[:, 1:1 + H, 1:1 + W]


# ------------------------------------------------------------------------------------------------ even-pixel subsample, NHWC
def subsample2(x):
    return x[:, ::2, ::2]


def subsample2_bwd(dxs):
    B, h, w, Cc = dxs.shape
    dx = torch.zeros(B, 2 * h, 2 * w, Cc, dtype=dxs.dtype)
    dx[:, ::2, ::2] = dxs
    return dx


# ------------------------------------------------------------------------------------------------ BatchNorm + add + ReLU, channels last
def add_relu_u(y, scale, shift, r, yd, scale_d, shift_d, dt):
    """u = y * scale + shift + R; R = r (form 1) or yd * scale_d + shift_d (form 2).  Returns (u, main, R)."""
    main = y.to(dt) * scale.to(dt) + shift.to(dt)
    R = r.to(dt) if r is not None else yd.to(dt) * scale_d.to(dt) + shift_d.to(dt)
    return main + R, main, R


def add_relu_apply(y, scale, shift, r, yd, scale_d, shift_d, dt):
    """(z, mag): z = max(0, u); mag = the larger of |main| and |R|, the terms of the element's last addition"""
    u, main, R = add_relu_u(y, scale, shift, r, yd, scale_d, shift_d, dt)
    return torch.relu(u), torch.maximum(main.abs(), R.abs())


def add_relu_du(dz, y, scale, shift, r, yd, scale_d, shift_d):
    """dU = dz * (u > 0) with u in float64 from the stored operands"""
    u, _, _ = add_relu_u(y, scale, shift, r, yd, scale_d, shift_d, torch.float64)
    return torch.where(u > 0, dz.double(), torch.zeros_like(u))


def add_relu_terms(du, x, mean, rstd, dt):
    """(dU, dU * xhat) in dt, xhat = (x - mean) * rstd"""
    d = du.to(dt)
    return d, d * (x.to(dt) - mean.to(dt)) * rstd.to(dt)


def bwd_coef(S1, S2, n, gamma, rstd):
    """fva_bn_bwd_finalize's table in float64: a = gamma * rstd, cb = -a * S2 / n, cc = -a * S1 / n"""
    a = gamma.double() * rstd.double()
    return a, -a * S2.double() / n, -a * S1.double() / n


def add_relu_dy(du, x, mean, rstd, a, cb, cc, dt):
    """(dY, mag): dY = a * dU + k1 * x + k2, k1 = cb * rstd, k2 = cc - k1 * mean"""
    k1 = cb.to(dt) * rstd.to(dt)
    k2 = cc.to(dt) - k1 * mean.to(dt)
    t1, t2 = a.to(dt) * du.to(dt), k1 * x.to(dt)
    return t1 + t2 + k2, torch.maximum(torch.maximum(t1.abs(), t2.abs()), k2.abs().expand_as(t1))


# ------------------------------------------------------------------------------------------------ the classifiers from stock modules
def _conv(cin, cout, k, stride=1):
    return nn.Conv2d(cin, cout, kernel_size=(k, k), stride=(stride, stride), padding=(k // 2, k // 2), bias=False)


class _Block(nn.Module):
    """One residual block; ``kind`` 'basic' (two 3x3, the stride on the first) or 'bottleneck' (1x1, 3x3 with the stride, 1x1 to 4 * mid;
    a shortcut convolution whenever the widths differ, also at stride 1)."""

    def __init__(self, kind, cin, mid, down, stride):
        super().__init__()
        self.kind = kind
        if kind == 'basic':
            cout = mid
            self.down = down
            self.conv1, self.bn1 = _conv(cin, mid, 3, stride), nn.BatchNorm2d(mid)
            self.conv2, self.bn2 = _conv(mid, cout, 3), nn.BatchNorm2d(cout)
        else:
            cout = mid * 4
            self.down = down or cin != cout
            self.conv1, self.bn1 = _conv(cin, mid, 1), nn.BatchNorm2d(mid)
            self.conv2, self.bn2 = _conv(mid, mid, 3, stride), nn.BatchNorm2d(mid)
            self.conv3, self.bn3 = _conv(mid, cout, 1), nn.BatchNorm2d(cout)
        self.relu = nn.ReLU(inplace=True)
        if self.down:
            self.downsample = nn.Sequential(_conv(cin, cout, 1, stride), nn.BatchNorm2d(cout))

    def units(self):
        """[(conv, bn)] of the main branch, the last one being the tail that takes the add"""
        u = [(self.conv1, self.bn1), (self.conv2, self.bn2)]
        return u + [(self.conv3, self.bn3)] if self.kind == 'bottleneck' else u


class StockResNet(nn.Module):
    """``act(u, info)`` and ``pool(x)`` default to ReLU and MaxPool2d(3, 2, 1); a test may pass its own to take decisions from elsewhere.
    info = {'name', 'x', 'conv', 'bn', 'y', 'short'}: the unit's input, modules, convolution output and, for a tail, the other summand's
    description (('identity', x) or ('conv', x, conv_d, bn_d, y_d)).  ``store(t)`` (default: the identity) is applied wherever the device
    writes a tensor in the compute dtype -- the images on their way into the patch matrix, every convolution output, every activation,
    the pooled vector in front of the fc layer -- and ``wround(w)`` to every weight a GEMM reads: a test emulates bf16 storage with them."""

    def __init__(self, name, in_channels=3, num_classes=1000, including_top=True):
        super().__init__()
        kind, blocks = BLOCKS[name]
        exp = 1 if kind == 'basic' else 4
        self.including_top = including_top
        self.conv1 = nn.Sequential(_conv(in_channels, 64, 7, 2), nn.BatchNorm2d(64), nn.ReLU(inplace=True))
        self.pool1 = nn.Sequential(nn.MaxPool2d(kernel_size=(3, 3), stride=(2, 2), padding=(1, 1)))
        planes = 64
        for stage, (n, mid) in enumerate(zip(blocks, (64, 128, 256, 512)), start=2):
            first = stage > 2
            layers = [_Block(kind, planes, mid, first, 2 if first else 1)]
            planes = mid * exp
            layers += [_Block(kind, planes, mid, False, 1) for _ in range(1, n)]
            setattr(self, f'res{stage}', nn.Sequential(*layers))
        if including_top:
            self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
            self.fc = nn.Linear(planes, num_classes)
        for m in self.modules():            # utils.initialize_weights of the reference, in module order
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
            elif isinstance(m, nn.Linear):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
                nn.init.constant_(m.bias, 0)

    def forward(self, x, act=None, pool=None, store=None, wround=None):
        act = act or (lambda u, info: F.relu(u))
        pool = pool or (lambda t: F.max_pool2d(t, 3, 2, 1))
        store = store or (lambda t: t)
        wround = wround or (lambda w: w)

        def run(conv, t):
            return store(F.conv2d(t, wround(conv.weight), None, conv.stride, conv.padding))

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
