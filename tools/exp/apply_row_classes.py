"""Row and tile classes of the batched apply kernel (csrc/kernels_dense_batch.hip: k_build_apply_meta, ApplyTileClass)
on R-MAT `scale`, from the lifted layout alone: no device is used.
    python tools/exp/apply_row_classes.py [scale]
Prints the rows with in-edges (n_nz), those of them with out-degree 0, the rows without in-edges that a sweep carries
(n_zin), and the 64-row tiles of each class as the kernel builds them."""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("personalized-pagerank-algorithms-on-neo4j_amd")

TILE = 64


def tile_classes(L):
    """(dead-end tiles, tiles without in-edges, plain tiles) by the kernel's rule: every one of a tile's 64 ordinals is
    a row with in-edges and out-degree 0; every one lies behind the rows with in-edges (the padding included)."""
    nz, zin = np.asarray(L["nz_rows"], dtype=np.int64), np.asarray(L["zin_rows"], dtype=np.int64)
    dout = np.diff(np.asarray(L["out_rp"], dtype=np.int64))
    n_nz, n_rows = nz.size, nz.size + zin.size
    n_tiles = (n_rows + TILE - 1) // TILE
    dead_row = np.zeros(n_tiles * TILE, dtype=bool)
    dead_row[:n_nz] = dout[nz] == 0
    no_in_row = np.arange(n_tiles * TILE) >= n_nz
    dead = dead_row.reshape(n_tiles, TILE).all(axis=1)
    no_in = no_in_row.reshape(n_tiles, TILE).all(axis=1)
    return dead, no_in, ~(dead | no_in)


def main():
    scale = int(sys.argv[1]) if len(sys.argv) > 1 else 22
    h = pkg.HostCsr.rmat(scale, 16, seed=1)
    L = pkg.lift_host(h)
    nz = np.asarray(L["nz_rows"], dtype=np.int64)
    dout = np.diff(np.asarray(L["out_rp"], dtype=np.int64))
    dead, no_in, plain = tile_classes(L)
    print("R-MAT %d: n %d, m %d, n_nz %d (out-degree 0: %d), n_zin %d; tiles %d: plain %d, dead-end %d, without "
          "in-edges %d" % (scale, h.n, h.m, nz.size, int((dout[nz] == 0).sum()), len(L["zin_rows"]), dead.size,
                           int(plain.sum()), int(dead.sum()), int(no_in.sum())))


if __name__ == "__main__":
    main()
