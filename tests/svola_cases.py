"""The shapes of the svola_convolution tests, shared by tests/test_gpu_svola.py (the kernels) and tests/test_svola_cpu.py (the
planner and the torch path), the seeded generator of the fuzz geometries, and a Python statement of how the host cuts an
axis into tiles (csrc/tl_svola.hip: cut_axis), written from the definition so that the CPU tests can pin the planner.

Why each shape from 8 on is there (kMaxSeg = 96 tile rows / columns and 65535 / C lenses per launch, kMaxGrid = 128):
    8-rows-long            99 tile rows: two row chunks, row_base = 96 in the second launch of every kernel
    9-cols-long            99 tile columns: two column chunks, col_base = 96
    10-cols-grid128        the grid at its limit along the columns, 255 tile columns in chunks of 96, 96, 63; first_c up to 252
    11-rows-grid128        the same along the rows, with PSFs shared by a batch of 2
    12-both-chunked        97 x 97 tiles: row_base and col_base non-zero in the same launch; the last chunk holds one tile
                           row, so the clamped copy of the tile table pads 95 entries
    13-z-chunks            C = 21846: 65535 // C = 2 lenses per launch, so b0 = 0, 2 in the three tile kernels and two launches
                           of the reduce with the workspace and g_psfs offset by two lenses
    13b-z-uneven           the same with B = 3: launches of 2 + 1 lenses (the last chunk shorter than the others)
    14-z-chunks-shared     13 with psf_batch = 1: one fold in the reduce over lenses that two launches wrote
    15-z-65535             C at its limit: one lens per launch, grid z = 65535 exactly
    16-halo-is-image       kh/2 == H, kw/2 == W: every pixel folds all 9 mirror terms, reflect() returns every index class
    17-halo-overlap-limit  oh + kh/2 == H and ow + kw/2 == W with an overlap larger than the patch core
    18-crowded-rows        H // gh == 0: patches of 2 oh rows, repeated patch starts, 120 patches over one row segment
    19-crowded             36 x 24 = 864 covering patches per tile: 216 passes of the four-at-a-time loop of the PSF backward
"""
import numpy as np

import svola_ref as ref

TILE = 32               # kTile of csrc/tl_svola.hip: the longest tile edge
MAX_SEG = 96            # kMaxSeg: tile rows / columns per launch

# B, H, W, C, grid, PSF, overlap, window, psf_batch
CASES = {
    "1-odd-boxcar": (2, 23, 29, 2, (2, 3), (5, 3), (2, 3), "boxcar", None),
    "1-odd-hann": (2, 23, 29, 2, (2, 3), (5, 3), (2, 3), "hann", None),
    "2-taps31": (1, 40, 40, 1, (1, 2), (31, 31), (0, 4), "boxcar", None),
    "3-tiles-hann": (1, 70, 131, 3, (3, 4), (7, 7), (5, 5), "hann", None),
    "4-cover3": (1, 24, 24, 1, (4, 4), (3, 3), (5, 5), "boxcar", None),
    "5-shared-psfs": (3, 23, 29, 2, (2, 3), (5, 3), (2, 3), "hann", 1),
    "6-degenerate": (1, 8, 8, 1, (1, 1), (1, 1), (0, 0), "boxcar", None),
    "8-rows-long": (1, 3100, 8, 1, (2, 1), (3, 3), (2, 1), "boxcar", None),
    "9-cols-long": (1, 8, 3100, 1, (1, 2), (3, 3), (1, 2), "hann", None),
    "10-cols-grid128": (1, 12, 384, 2, (1, 128), (3, 5), (0, 1), "hann", None),
    "11-rows-grid128": (2, 384, 12, 1, (128, 1), (5, 3), (1, 0), "boxcar", 1),
    "12-both-chunked": (1, 147, 3100, 1, (49, 1), (3, 3), (1, 0), "boxcar", None),
    "13-z-chunks": (4, 3, 3, 21846, (1, 1), (3, 3), (0, 0), "boxcar", None),
    "13b-z-uneven": (3, 3, 3, 21846, (1, 1), (3, 3), (0, 0), "boxcar", None),
    "14-z-chunks-shared": (4, 3, 3, 21846, (1, 1), (3, 3), (0, 0), "hann", 1),
    "15-z-65535": (2, 2, 2, 65535, (1, 1), (1, 1), (0, 0), "boxcar", None),
    "16-halo-is-image": (1, 15, 15, 1, (1, 1), (31, 31), (0, 0), "boxcar", None),
    "17-halo-overlap-limit": (1, 16, 9, 2, (2, 1), (9, 5), (12, 7), "hann", None),
    "18-crowded-rows": (1, 8, 9, 1, (128, 1), (3, 3), (4, 0), "hann", None),
    "19-crowded": (2, 6, 7, 2, (40, 24), (3, 5), (3, 4), "hann", None),
}
# tile rows x tile columns of the chunked shapes: more than MAX_SEG along an axis is more than one launch along it
TILE_COUNTS = {"8-rows-long": (99, 1), "9-cols-long": (1, 99), "10-cols-grid128": (1, 255), "11-rows-grid128": (255, 1),
               "12-both-chunked": (97, 97)}

FUZZ_SEED, FUZZ_DRAWS, FUZZ_MAX_SKIPPED = 20261018, 64, 64 // 3


def cut_tiles(size, grid, overlap):
    """One axis: (number of tiles, [tiles under each patch]).  The patch bounds that fall strictly inside the centre
    [overlap, overlap + size) of the frame split it into cells, a cell of n pixels becomes ceil(n / TILE) tiles, and a patch
    lies over the tiles of every cell it contains."""
    p0, p1, _ = ref.patch_starts(size, grid, overlap)
    lo, hi = overlap, overlap + size
    marks = sorted({lo, hi} | {int(v) for v in np.concatenate((p0, p1)) if lo < v < hi})
    cells = [(s, e, -(-(e - s) // TILE)) for s, e in zip(marks[:-1], marks[1:])]
    under = [sum(t for s, e, t in cells if p0[i] <= s and e <= p1[i]) for i in range(grid)]
    return sum(t for _, _, t in cells), under


def workspace_bytes(B, H, W, C, grid, k, overlap):
    """What tl_svola_workspace_bytes must return: the larger of the PSF backward's per-tile partials [B C][N][slots][kh kw] and
    the image backward's extended frame [B C][H + kh - 1][W + kw - 1], floats, plus 256 bytes.  slots = the most tiles under
    one patch row x the most under one patch column."""
    slots_r = max(1, max(cut_tiles(H, grid[0], overlap[0])[1]))
    slots_c = max(1, max(cut_tiles(W, grid[1], overlap[1])[1]))
    part = B * C * grid[0] * grid[1] * slots_r * slots_c * k[0] * k[1] * 4
    ext = B * C * (H + k[0] - 1) * (W + k[1] - 1) * 4
    return max(part, ext) + 256


def fuzz_draws():
    """The 64 seeded draws of the fuzz tests, in order: [(index, (B, H, W, C, grid, PSF, overlap, window))]."""
    rng = np.random.default_rng(FUZZ_SEED)
    draws = []
    for t in range(FUZZ_DRAWS):
        H, W = (int(rng.integers(1, 80)) for _ in range(2))
        gh, gw = (int(rng.integers(1, 9)) for _ in range(2))
        kh, kw = (2 * int(rng.integers(0, 8)) + 1 for _ in range(2))
        oh, ow = (int(rng.integers(0, 9)) for _ in range(2))
        B, C = int(rng.integers(1, 3)), int(rng.integers(1, 4))
        draws.append((t, (B, H, W, C, (gh, gw), (kh, kw), (oh, ow), ("boxcar", "hann")[t % 2])))
    return draws


def fuzz_survivors(geometry):
    """The draws that svola_convolution accepts, and how many were skipped.  `geometry` is imaging.svola_geometry (its
    ValueError for a pixel that no patch covers is one of the reasons to skip)."""
    kept = []
    for t, (B, H, W, C, (gh, gw), (kh, kw), (oh, ow), win) in fuzz_draws():
        if oh + kh // 2 > H or ow + kw // 2 > W or H // gh < 1 or W // gw < 1:
            continue
        try:
            geometry(H, W, gh, gw, oh, ow, win)
        except ValueError:
            continue
        kept.append((t, (B, H, W, C, (gh, gw), (kh, kw), (oh, ow), win)))
    return kept, FUZZ_DRAWS - len(kept)
