"""Writes tests/golden/frame_store.npz: what PIL ITSELF makes of seeded uint8 frames the way the event loaders treat their paired camera
frame -- Image.resize((Wr, Hr)) WITHOUT a filter argument (bicubic on 'RGB' and 'L'), then convert('L') for an RGB frame -- at small
size pairs, so that a machine without PIL can still compare with PIL's bits.  The inputs are not stored: tests/frame_store_ref.py
makes them again from the seed (make_image).  Imports PIL, numpy and that module only.  Run from the repository root:
python tests/golden/make_golden_frame_store.py"""
import os
import sys

import numpy as np
from PIL import Image

import PIL

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests.frame_store_ref import make_image  # noqa: E402

# (source shape, (Hr, Wr)): both sides shrink / grow, one side unchanged, the DDD17 ratio, a shrink by more than 7
CASES = [((37, 300, 3), (29, 277)), ((23, 41), (31, 59)), ((30, 64, 3), (28, 64)), ((30, 64, 3), (30, 50)), ((26, 35), (26, 36)),
         ((37, 53, 3), (29, 41)), ((37, 53), (61, 90)), ((64, 80, 3), (9, 11))]
SEED = 20241021


def main():
    out = {'cases': np.array([list(s) + [0] * (3 - len(s)) + list(o) for s, o in CASES], dtype=np.int32), 'seed': np.array(SEED),
           'pil_version': np.array(PIL.__version__)}
    for i, (shape, (Hr, Wr)) in enumerate(CASES):
        img = make_image(shape, SEED + i)
        r = Image.fromarray(img).resize((Wr, Hr))
        out[f'out_{i}'] = np.array(r.convert('L') if img.ndim == 3 else r)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'frame_store.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
