"""The specification of mf_ring_exchange_u8 (include/meshflow_hip.h; `ops.ring_exchange`): one tick of a ring of owed frames, in NumPy.
ring (B, lag, ...): frame t of stream b lives in slot t mod lag while it is owed; new (K, ...): one new frame per row; rows (K, 3) ints:
(id, slot, out_row) per row, the ids distinct.  A row with out_row >= 0 hands out what its slot holds before the new frame takes the slot."""
import numpy as np


def exchange(ring, new, rows, M):
    """(the new ring, out (M, ...)); the arguments are left as they are."""
    rows = np.asarray(rows).reshape(-1, 3)
    ring, emit = ring.copy(), rows[:, 2] >= 0
    out = np.empty((M,) + new.shape[1:], dtype=new.dtype)
    out[rows[emit, 2]] = ring[rows[emit, 0], rows[emit, 1]]
    ring[rows[:, 0], rows[:, 1]] = new
    return ring, out


def tick_rows(ids, seen, lag):
    """The rows of a tick in which stream ids[r], with seen[ids[r]] frames so far, pushes one more: its frame `seen` takes slot seen mod lag,
    which holds frame seen - lag once the stream has `lag` frames; the rows that hand a frame out are numbered in row order.  Returns
    (rows (K, 3) int32, M)."""
    rows, M = [], 0
    for b in ids:
        emits = seen[b] >= lag
        rows.append((b, seen[b] % lag, M if emits else -1))
        M += int(emits)
    return np.array(rows, dtype=np.int32).reshape(-1, 3), M
