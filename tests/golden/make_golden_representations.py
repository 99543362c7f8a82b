"""
Generate tests/golden/event_histogram.pt by IMPORTING THE REFERENCE (read-only) on CPU, as make_golden.py does for voxel.pt: the
output of the reference's generate_event_histogram (datasets/data_util.py:17-35) on a few thousand synthetic IN-RANGE events at
48 x 64.  Data only: the events are regenerated from their seeds (oracle.ess_oracle.synth_events with border=0), the file holds the
histograms.  Run:   python tests/golden/make_golden_representations.py

Out-of-range events are left out on purpose: the reference neither checks nor drops them (x + width * y wraps into a neighbouring
row or raises), which the ingest does not reproduce.  data_util uses the removed alias np.int: restored here.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = '/root/reference'
sys.path.insert(0, ROOT)
from oracle import ess_oracle as O  # noqa: E402

H, W = 48, 64
CASES = [(5000, 21, False), (3000, 22, True), (1, 23, False), (4096, 24, True)]  # (n, seed, polarity as -1 / +1)


def histogram_events(n, seed, pm):
    """-> [n, 4] float64 rows (x, y, t, p) as generate_event_histogram reads them: integral pixels inside H x W, p in {0, 1} or,
    pm, {-1, +1}"""
    x, y, pol, t = O.synth_events(n, H, W, seed, border=0.0)
    p = pol.double() * 2 - 1 if pm else pol.double()
    return torch.stack([x.double().floor(), y.double().floor(), t.double(), p], 1).numpy()


def main():
    if not hasattr(np, 'int'):
        np.int = int
    spec = importlib.util.spec_from_file_location('ref_data_util', os.path.join(REF, 'datasets/data_util.py'))
    du = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(du)
    cases = []
    for n, seed, pm in CASES:
        ev = histogram_events(n, seed, pm)
        assert ev[:, 0].min() >= 0 and ev[:, 0].max() < W and ev[:, 1].min() >= 0 and ev[:, 1].max() < H
        hist = torch.from_numpy(du.generate_event_histogram(ev.copy(), (H, W)))
        assert hist.dtype == torch.float32 and tuple(hist.shape) == (2, H, W) and float(hist.sum()) == n
        cases.append(dict(n=n, seed=seed, pm=pm, histogram=hist.clone()))
    path = os.path.join(HERE, 'event_histogram.pt')
    torch.save(dict(H=H, W=W, cases=cases), path)
    print(f'event_histogram: {os.path.getsize(path) / 1e3:.0f} kB')


if __name__ == '__main__':
    main()
