"""tests/randaug_restatement.py pinned on hand-computed cases, the excused / left-out shares of the GPU test's cases counted on the CPU, the
new C symbols and their argument checks, and the Python surface (construction, refusals of CPU tensors, the alias)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import randaug_restatement as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ['fva_randaug_plan', 'fva_randaug_plan_fixed', 'fva_randaug_workspace', 'fva_randaug_stats', 'fva_randaug_apply', 'fva_random_erase']


def test_equalize_table_of_a_known_histogram():
    # 16 pixels: 4 x 10, 4 x 20, 8 x 30 -> step = (16 - 8) // 255 = 0: identity; 1024 pixels at 4 levels: step = (1024 - 256) // 255 = 3
    hist = np.zeros(256, np.int64)
    hist[[10, 20, 30]] = 4, 4, 8
    assert rr.equalize_table(hist, 16) is None
    hist[:] = 0
    hist[[0, 100, 200, 255]] = 256
    lut = rr.equalize_table(hist, 1024)
    # lut[i] = min(255, (cumsum[i - 1] + 1) // 3): 0 at 0, 257 // 3 = 85 up to 100, 513 // 3 = 171 up to 200, 769 // 3 = 256 -> 255 above
    assert lut[0] == 0 and lut[1] == 85 and lut[100] == 85 and lut[101] == 171 and lut[200] == 171 and lut[201] == 255 and lut[255] == 255


def test_autocontrast_ends_posterize_masks_and_blend():
    img = np.zeros((4, 4, 3), np.uint8)
    img[..., 0] = np.arange(16).reshape(4, 4) * 10 + 50            # 50 .. 200
    img[..., 1] = 99                                                # constant: identity
    img[..., 2] = np.where(np.arange(16).reshape(4, 4) % 2, 30, 40)
    out, e, s = rr.apply_op(img, 'AutoContrast', 0)
    assert not e.any() and not s.any()                                # ends 50 and 200: 0 and 255; (60 - 50) * 255 // 150 = 17
    assert out[0, 0, 0] == 0 and out[3, 3, 0] == 255 and out[0, 1, 0] == 10 * 255 // 150 and (out[..., 1] == 99).all()
    assert set(out[..., 2].ravel()) == {0, 255}
    assert [rr.posterize_mask(b) for b in (8, 7, 4, 1, 0)] == [0xFF, 0xFE, 0xF0, 0x80, 0x00]
    assert (rr.apply_op(img, 'Posterize', 4)[0] == (img & 0xF0)).all()
    # Brightness: trunc(1.5 x) clamped; 200 -> 255; excused where 1.5 x is an integer (even x), never at v == 0
    out, e, _ = rr.apply_op(img, 'Brightness', 0.5)
    assert out[0, 0, 0] == 75 and out[3, 3, 0] == 255 and out[0, 0, 1] == 148 and e[0, 0, 0] and not e[3, 3, 0] and not e[0, 0, 1]
    assert not rr.apply_op(img, 'Brightness', 0.0)[1].any()
    assert rr.grey(np.array([[[255, 255, 255], [10, 200, 30]]], np.uint8)).tolist() == [[254, 123]]     # the weights sum to 0.9999


def test_rotation_by_90_degrees_translation_and_sharpness_on_small_images():
    img = np.arange(75, dtype=np.uint8).reshape(5, 5, 3)
    out, _, s = rr.apply_op(img, 'Rotate', 90.0)
    assert (out == np.rot90(img, 1)).all() and not s.any()          # source = R(90) (p - c) + c: out[y, x] = in[x, 4 - y]
    out, _, _ = rr.apply_op(img, 'TranslateX', 2.0, (1, 2, 3))
    assert (out[:, 2:] == img[:, :3]).all() and (out[:, :2] == (1, 2, 3)).all()
    flat = np.full((4, 4, 3), 50, np.uint8)
    flat[1, 1] = 63                                                  # the sum at (1, 1): 8 * 50 + 5 * 63 = 715 -> 55; at (1, 2): 12 * 50 + 63 = 663 -> 51
    assert rr.smoothed(flat)[1, 1, 0] == 55 and rr.smoothed(flat)[1, 2, 0] == 51
    out, _, _ = rr.apply_op(flat, 'Sharpness', 0.5)                  # 1.5 * 63 - 0.5 * 55 = 67; 1.5 * 50 - 0.5 * 51 = 49.5 -> 49; the border stays
    assert out[1, 1, 0] == 67 and out[1, 2, 0] == 49 and (out[0] == 50).all() and (out[:, 3] == 50).all()


def test_the_gpu_cases_stay_under_the_cap_by_the_restatement_alone():
    import test_gpu_randaug as tg
    images = [rr.canvases(B, H, W, 100 + i) for i, (B, H, W) in enumerate(tg.SHAPES)]
    for op, vals in tg.CASES.items():
        for v in vals:
            marks = [rr.apply_op(img, op, float(np.float32(v)), tg.FILL)[1:] for batch in images for img in batch]
            marked, total = sum(int((e | s).sum()) for e, s in marks), sum(e.size for e, _ in marks)
            assert marked <= 0.01 * total, (op, v, marked, total)


@pytest.fixture(scope='module')
def built():
    import __graft_entry__ as ge
    ge.build()
    from fastvision_amd import _lib
    return _lib


def test_version_symbols_and_argument_checks(built):
    lib = built.load()
    assert lib.fva_version() >= 14
    hdr = open(os.path.join(ROOT, 'include', 'fastvision_amd.h')).read()
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in NEW:
        assert f'{name}(' in hdr and f'`{name}`' in doc and hasattr(lib, name) and name in built.PROTOTYPES, name
    assert lib.fva_randaug_workspace(2) == 4 * (4 + 2 * 2 * 1024) and lib.fva_randaug_workspace(0) == 0
    p, q = C.c_void_p(4096), C.c_void_p(1 << 20)                       # never dereferenced: both fail in the argument checks
    assert lib.fva_randaug_apply(p, p, p, 0, 2, 2, 8, 8, 0, p, None) == -1 and b'out of place' in lib.fva_last_error()
    assert lib.fva_randaug_plan(p, 2, 5, 9, 31, 8, 8, 0x3FFF, q, None) == -1 and b'num_ops' in lib.fva_last_error()


def test_python_surface_imports_constructs_and_refuses_cpu_tensors():
    import fastvision
    import fastvision_amd
    from fastvision_amd import RandAugment, RandomErasing
    from fastvision_amd.augment import OPS
    assert OPS == rr.OPS and fastvision.RandAugment is RandAugment and fastvision_amd.RandomErasing is RandomErasing
    torch.manual_seed(31)
    aug = RandAugment()
    assert (aug.num_ops, aug.magnitude, aug.num_magnitude_bins, aug.fill, aug.op_mask) == (2, 9, 31, (0, 0, 0), 0x3FFF)
    assert aug._state.tolist() == [31, 0, 0, 0] and not aug.state_dict()
    assert RandAugment(ops=['Rotate', 'Equalize'], seed=4).op_mask == (1 << 5) | (1 << 13)
    for bad in (dict(num_ops=0), dict(num_ops=5), dict(magnitude=31), dict(ops=['Blur']), dict(ops=[]), dict(fill=(1, 2)), dict(fill=300)):
        with pytest.raises(ValueError):
            RandAugment(**bad)
    with pytest.raises(ValueError):
        RandomErasing(scale=(0.5, 0.2))
    canv, batch = torch.zeros(2, 8, 8, 3, dtype=torch.uint8), torch.zeros(2, 3, 8, 8)
    with pytest.raises(RuntimeError):
        aug(canv)
    with pytest.raises(RuntimeError):
        RandomErasing()(batch)
    assert aug.eval()(canv) is canv and RandomErasing().eval()(batch) is batch
