"""The row frame the spot-merit kernels share (torchoptics_amd/csrc/tl_rows.h), restated in Python: the launch plan, the size of
the partials' workspace, the grid-y launches and a CPU emulation of the order in which a row's terms are added.  focus_ref,
enclosed_ref, zfit_ref and mtf_ref import it.  It shares no code with the package."""
import numpy as np

BLOCK, VEC, TARGET_BLOCKS, MAX_Y = 256, 4, 2048, 65535
CHUNK = BLOCK * VEC


def plan(rows, P):
    """(nbx, R) of the kernels: blocks per row and steps of 1024 rays per block, aiming at 2048 blocks."""
    chunks = -(-P // CHUNK)
    want = max(1, -(-TARGET_BLOCKS // rows))
    R = -(-chunks // min(chunks, want))
    return -(-chunks // R), R


def workspace_bytes(F, P, W, n):
    """One partial of n doubles per block; 0 for the sizes the calls refuse."""
    if min(F, P, W) < 1 or F * W >= 2 ** 31 or F >= 2 ** 31 or W >= 2 ** 31 or P >= 2 ** 31:
        return 0
    return F * W * plan(F * W, P)[0] * n * 8


def launches(rows):
    """(row0, rows of the launch) of the grid-y chunks."""
    return [(r0, min(MAX_Y, rows - r0)) for r0 in range(0, rows, MAX_Y)]


def emulate_sums(t, aligned, batch=2048):
    """[rows, K]: the fp64 terms t [rows, P, K] added in the kernels' order: per lane in the order of its loop (four consecutive
    rays per step of 1024 where aligned[row], else one per step of 256), the butterfly over the 64 lanes of a wave, the four waves
    in order, the row's partials in order."""
    rows, P, K = t.shape
    nbx, R = plan(rows, P)
    out = np.zeros((rows, K))
    lane, xor = np.arange(BLOCK), np.arange(64)
    for r0 in range(0, rows, batch):
        for vec in (False, True):
            sel = r0 + np.flatnonzero(np.asarray(aligned[r0:r0 + batch]) == vec)
            if not len(sel):
                continue
            acc = np.zeros((len(sel), K))
            for bx in range(nbx):
                first, last = bx * R * CHUNK, min((bx + 1) * R * CHUNK, P)
                lanes = np.zeros((len(sel), BLOCK, K))
                steps = [first + k * CHUNK + VEC * lane + j for k in range(R) for j in range(VEC)] if vec else \
                        [first + k * BLOCK + lane for k in range(R * VEC)]
                for idx in steps:
                    m = idx < last
                    if m.any():
                        lanes[:, m] += t[sel][:, idx[m]]
                w = lanes.reshape(len(sel), BLOCK // 64, 64, K)
                for o in (32, 16, 8, 4, 2, 1):
                    w = w + w[:, :, xor ^ o]
                part = np.zeros((len(sel), K))
                for q in range(BLOCK // 64):
                    part = part + w[:, q, 0]
                acc = acc + part
            out[sel] = acc
    return out
