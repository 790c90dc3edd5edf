"""Host-side records for the per-record GPU tests (test_gpu_issue.py, test_gpu_soft.py): a row is key[32] | nonce16[16] | msg[msg_bytes], zero-padded to
the stride.  The byte offsets of the record head are written here and nowhere else in those tests."""
import numpy as np


def _split(rows, mb):
    return [(bytes(r[:32]), bytes(r[32:48]), bytes(r[48:48 + mb])) for r in rows]


def make_records(B, mb, seed, stride=None):
    """(host rows uint8 [B, stride], [(key, nonce, msg)])"""
    rs = np.random.RandomState(seed)
    stride = (48 + mb + 15) // 16 * 16 if stride is None else stride
    rows = np.zeros((B, stride), dtype=np.uint8)
    rows[:, :48 + mb] = rs.randint(0, 256, (B, 48 + mb), dtype=np.uint8)
    return rows, _split(rows, mb)


def counter_carry_rows(rows, mb):
    """The block counter carries inside the row: the 32-bit counter of image 0 at block 1, the 64-bit counter of image 1 wraps at block 2
    (the pattern of test_embed_identity_block_counter_carries_inside_the_lattice) -> the records again"""
    rows[0, 32:36] = 0xFF
    rows[1, 32:40] = 0xFF
    rows[1, 32] = 0xFE
    return _split(rows, mb)
