"""GPU tier of the label's side of the training window (csrc/voxel_ingest.hip: ess_label_window): nearest resize by the exact integer
rule sy = min(dy * Hs // Hr, Hs - 1), then the flip and the window of hip.event_grid_finish_window with the same clamps.  Every
element is compared against a numpy restatement of that rule; the values pass unchanged (0..18 and 255)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import test_hip_event_columns as C  # noqa: E402  (guards)
from tests import test_hip_multi_stream as M  # noqa: E402  (guarded buffers)

DEV = M.DEV
SIZES = {'7x5->5x9': ((7, 5), (5, 9)), '11x16->12x16': ((11, 16), (12, 16)), 'identity': ((6, 8), (6, 8))}


def restate(src, resize, words, h, w):
    """src uint8 [n, Hs, Ws] (numpy) -> int64 [n, h, w]: the integer rule, the flip, the window, with the device's clamps"""
    n, Hs, Ws = src.shape
    Hr, Wr = resize
    sy = np.minimum(np.arange(Hr) * Hs // Hr, Hs - 1)
    sx = np.minimum(np.arange(Wr) * Ws // Wr, Ws - 1)
    out = np.empty((n, h, w), np.int64)
    for i in range(n):
        flip, y0, x0 = (int(v) for v in words[i][:3])
        y0, x0 = min(max(y0, 0), Hr - h), min(max(x0, 0), Wr - w)
        g = src[i][sy][:, sx]
        if flip != 0:
            g = g[:, ::-1]
        out[i] = g[y0:y0 + h, x0:x0 + w]
    return out


def _labels(n, hw, seed):
    """every value 0..18 and 255 occurs in every sample"""
    g = np.random.default_rng(seed)
    values = np.array(list(range(19)) + [255], dtype=np.uint8)
    lab = values[g.integers(0, len(values), (n,) + hw)]
    flat = lab.reshape(n, -1)
    flat[:, :len(values)] = values
    return lab


def _run(src, resize, words, h, w):
    from ess_amd import hip
    n = src.shape[0]
    buf, out = M._guarded((n, h, w), torch.int64)
    got = hip.label_window(torch.from_numpy(src).to(DEV), out, torch.tensor(words, dtype=torch.int32, device=DEV), resize=resize)
    # (C._guards_intact sizes the destination as fp32 elements: an int64 destination counts twice)
    assert got is out and C._guards_intact(buf, out.view(torch.float32))
    return out.cpu().numpy()


@pytest.mark.parametrize('size', list(SIZES))
@pytest.mark.parametrize('n', [1, 3])
def test_every_element_against_the_integer_rule(size, n):
    """whole and partial windows, both flips, per-sample words; out-of-range words give their clamped values; 0..18 and 255 survive"""
    (Hs, Ws), (Hr, Wr) = SIZES[size]
    src = _labels(n, (Hs, Ws), seed=n + Hs)
    if (Hs, Ws) == (Hr, Wr):
        assert (restate(src, (Hr, Wr), [[0, 0, 0, 0]] * n, Hr, Wr) == src).all()
    windows = [(Hr, Wr), (Hr - 2, Wr - 3), (1, 1), (Hr - 1, 4)]
    for h, w in windows:
        tables = [[[(i + k) % 2, (i * 2 + k) % (Hr - h + 1), (i * 3 + 2 * k) % (Wr - w + 1), 0] for i in range(n)] for k in range(2)]
        tables.append([[7, -3, 10 ** 6, 0], [0, 10 ** 6, -5, -1], [-1, (1 << 31) - 1, -(1 << 31), 0]][:n])
        for words in tables:
            got = _run(src, (Hr, Wr), words, h, w)
            want = restate(src, (Hr, Wr), words, h, w)
            assert (got == want).all(), (size, n, (h, w), words)
            assert got.dtype == np.int64 and set(np.unique(got)) <= set(range(19)) | {255}
    whole = _run(src, (Hr, Wr), [[0, 0, 0, 0]] * n, Hr, Wr)
    if Hr >= Hs and Wr >= Ws:  # (an upscale keeps every source pixel)
        assert set(np.unique(whole)) == set(range(19)) | {255}


def test_the_presets_rules_agree_with_the_double_rule():
    """at the loaders' label sizes the integer rule gives the index floor(d * (1 / (dst / src))) in doubles gives (cv2's INTER_NEAREST
    expression; parity with cv2 itself stays unpinned), for every d; and one 440 x 640 -> 448 x 640 label runs at full size"""
    for src, dst in ((440, 448), (640, 640), (346, 352), (480, 448)):
        d = np.arange(dst)
        rule = np.minimum(d * src // dst, src - 1)
        dbl = np.minimum(np.floor(d * (1.0 / (dst / src))).astype(np.int64), src - 1)
        assert (rule == dbl).all(), (src, dst)
    lab = _labels(1, (440, 640), seed=5)
    words = [[1, 0, 0, 0]]
    assert (_run(lab, (448, 640), words, 448, 640) == restate(lab, (448, 640), words, 448, 640)).all()
