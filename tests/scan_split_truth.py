"""The zone rule of the main scan launch (eps_amd.scan.lean_columns / zone_order), restated with plain loops in numpy.

A column list is cut into GENERAL | LEAN | LIGHT, each zone in the list's order.  A column is LEAN when it is not light, has at most
256 rows, every one of its plan records is direct-16 (kind bits 11), direct-32 (10) or packed (01) -- none a two-word hash piece
(00) -- and every piece fits one range of the kernel's unit bitmap: paths + 3 x rows <= 4 x 8192 (a row adds at most 3/4 of a
4-entry unit beyond its share of the paths).  The record layout is the plan table's: word 0 = paths | kind << 30."""
import numpy as np

UBITS = 8192
ROWS = 256


def lean_ok(rows, pptr, recs):
    """bool per node: ``rows`` [N], ``pptr`` [N + 1], ``recs`` [P, 4] (non-negative integers)."""
    rows, pptr, recs = np.asarray(rows, np.int64), np.asarray(pptr, np.int64), np.asarray(recs, np.int64).reshape(-1, 4)
    ok = np.zeros(len(rows), bool)
    for v in range(len(rows)):
        good = rows[v] <= ROWS
        for i in range(pptr[v], pptr[v + 1]):
            kind, paths = recs[i, 0] >> 30, recs[i, 0] & 0x3FFFFFFF
            if kind == 0 or paths + 3 * rows[v] > 4 * UBITS:
                good = False
        ok[v] = good
    return ok


def zones(columns, light, lean):
    """(the list in zone order, lean_from, light_from); ``light`` / ``lean`` are flags per ENTRY of ``columns``, light wins."""
    columns = list(columns)
    gen = [c for c, li, le in zip(columns, light, lean) if not li and not le]
    mid = [c for c, li, le in zip(columns, light, lean) if not li and le]
    lit = [c for c, li in zip(columns, light) if li]
    return gen + mid + lit, len(gen), len(gen) + len(mid)
