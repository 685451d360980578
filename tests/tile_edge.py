"""Lists cut to an exact length around the 1024-item tile of the frame index, shared by the merger's and
the unfolder's tests."""
import numpy as np

TILE_EDGE_SIZES = (1023, 1024, 1025, 2048)   # at 1024 and 2048 item i == n is alone in a tile of its own


def thin_to(recs, n, seed):
    """n records of an ordered list, its last record among them, in list order."""
    assert len(recs) > n
    keep = np.sort(np.random.default_rng(seed).choice(len(recs) - 1, n - 1, replace=False))
    return recs[np.append(keep, len(recs) - 1)]
