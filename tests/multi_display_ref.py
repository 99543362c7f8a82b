"""The steered auto-HDR step (ess_recon_post_bounds_steered) restated on the host: R history rows, each a recon_post_ref.History(1,
size); per call N slots, each with an image, a mode word and a history row.  A row is updated only by a TAKE / ZERO slot, and reset
first on ZERO; every other slot -- HOLD, any other word, a row outside [0, R) -- changes nothing and yields no bounds.

Also here: the three mutants the CPU tier proves its schedules can see, and the schedules both tiers run (images: R.hdr_images();
the slot's image is that call's image of its row, a padded slot gets image 0)."""
import numpy as np

from tests import recon_post_ref as R

HOLD, TAKE, ZERO = 0, 1, 2
H, T, Z = HOLD, TAKE, ZERO
PAD = -2  # (run_segmentation.SCATTER_SKIP: the row of a padded slot)


class Steered:
    """Mutants: hold_pushes -- a skipped slot with a row in range pushes anyway; zero_is_take -- a restart does not empty the history;
    slot_as_row -- the slot number is used as the history row."""

    def __init__(self, n_rows, filter_size, hold_pushes=False, zero_is_take=False, slot_as_row=False):
        self.rows = [R.History(1, filter_size) for _ in range(n_rows)]
        self.hold_pushes, self.zero_is_take, self.slot_as_row = hold_pushes, zero_is_take, slot_as_row

    def counts(self):
        return [len(h.held[0]) for h in self.rows]

    def update(self, img, w, amount, mode, rows=None):
        """img float32 [N, 1, Hs, Ws] -> (bounds float32 [N, 2], taken bool [N]); bounds of a slot that is not taken are NaN"""
        N = img.shape[0]
        out = np.full((N, 2), np.nan, dtype=R.F32)
        taken = np.zeros(N, dtype=bool)
        for n in range(N):
            r = n if (rows is None or self.slot_as_row) else int(rows[n])
            if not 0 <= r < len(self.rows):
                continue
            if mode[n] not in (TAKE, ZERO):
                if self.hold_pushes:
                    self.rows[r].update(img[n:n + 1], w, amount)
                continue
            if mode[n] == ZERO and not self.zero_is_take:
                self.rows[r].reset()
            out[n] = self.rows[r].update(img[n:n + 1], w, amount)[0]
            taken[n] = True
        return out, taken


# ---------------------------------------------------------------------------------------------- the schedules of both tiers
# ride-along: N = R = 3, identity rows, 7 calls.  Every row is held at least once and taken again; rows 0 and 2 are each restarted once
# while they hold >= 2 entries (row 0 in call 4 with 3 entries, row 2 in call 5 with 3).
RIDE_ALONG = [
    (None, [T, T, T]),
    (None, [T, H, T]),
    (None, [H, T, T]),
    (None, [T, T, H]),
    (None, [Z, H, T]),
    (None, [T, T, Z]),
    (None, [T, T, T]),
]
# compact: N = 2 slots over R = 3 rows
COMPACT = [
    ([0, 2], [T, T]),
    ([2, PAD], [T, H]),
    ([1, 0], [T, T]),
    ([2, 0], [Z, T]),
    ([2, 1], [H, T]),
    ([2, 0], [T, Z]),
    ([0, 2], [T, T]),
]
N_ROWS = 3


def slot_images(call, rows, n_slots):
    """the images of one call's slots: that call's hdr image of the slot's row (a padded slot: of row 0)"""
    imgs = R.hdr_images()[call]
    idx = list(range(n_slots)) if rows is None else [r if 0 <= r < imgs.shape[0] else 0 for r in rows]
    return np.ascontiguousarray(imgs[idx])


def run(schedule, filter_size, w, amount, **mutant):
    """-> per call (bounds [N, 2], taken [N], counts per row after the call)"""
    st = Steered(N_ROWS, filter_size, **mutant)
    out = []
    for t, (rows, mode) in enumerate(schedule):
        b, taken = st.update(slot_images(t, rows, len(mode)), w, amount, mode, rows)
        out.append((b, taken, st.counts()))
    return out


def taken_bits_differ(a, b):
    """two runs of one schedule: does any bounds bit of a slot the FIRST run takes differ?"""
    for (ba, ta, _), (bb, _, _) in zip(a, b):
        if (ba[ta].view(np.uint32) != bb[ta].view(np.uint32)).any():
            return True
    return False
