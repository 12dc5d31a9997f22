"""Cases whose operands' BYTE OFFSETS straddle given marks -- 2^31 and 2^32 on the GPU (tests/test_gpu_large_offsets.py), a few
KiB on the CPU (tests/test_large_offset_cases_host.py runs the same builders on CPU tensors in milliseconds).  A plain helper
module (no fixtures).

Two builders.  ``TallCase``: a table of many rows whose row index x leading dimension crosses the marks.  ``LongCSR``: a
directed CSR pattern whose col / val entry offsets cross them.  Both are periodic BALLAST -- one small block of exactly
representable values, broadcast over the operand by strided copies on the operand's own device -- with a few hundred LIVE rows
of seeded random data written over it; the host keeps the live rows alone.  Each builder also gives the COMPACTED TWIN: the same
live rows in a small operand at low offsets, ids remapped monotonically (every neighbour list keeps its order), on which the
float64 truths of the kernels' own helper modules (layer_truth, pair_score_truth, weighted_truth) are computed."""
import numpy as np
import scipy.sparse as ssp
import torch

import pair_score_truth as pt

GPU_MARKS = (1 << 31, 1 << 32)
SENTINEL = 0x7FC5A5A5                            # layer_truth.SENTINEL: the word an ``out`` buffer is filled with


# ====================================================================================================================
# tall tables
# ====================================================================================================================
def tall_rows(marks, pitch, margin_rows=160):
    """-> (n_rows, roles) for rows of ``pitch`` bytes.  roles: 'first' -> 0; ('below', m) -> the last row that ends at or below
    byte m; ('at', m) -> the row that contains byte m or starts at it; ('after', m) -> the next one; 'last' -> n_rows - 1.
    n_rows is the smallest count whose last row starts beyond max(marks) + margin_rows * pitch."""
    assert pitch > 0 and min(marks) >= pitch
    roles = {"first": 0}
    for m in marks:
        at = m // pitch
        roles[("below", m)], roles[("at", m)], roles[("after", m)] = at - 1, at, at + 1
    n_rows = (max(marks) + margin_rows * pitch) // pitch + 2
    roles["last"] = n_rows - 1
    return n_rows, roles


def ballast_values(rows, width):
    """The ballast of table rows ``rows`` (already reduced modulo the block): multiples of 1/8 in [-3.75, 3.75], float32.
    (Exact in float32 and in bfloat16; signs mixed.)"""
    r = np.asarray(rows, np.int64)[:, None]
    j = np.arange(width, dtype=np.int64)[None, :]
    return (((r * 31 + j * 7) % 61 - 30) / 8.0).astype(np.float32)


def fill_periodic(table, block):
    """table[r] = block[r % len(block)] for every row of a 2-D (row-strided) or 1-D tensor: ONE broadcast copy over the whole
    blocks and one copy of the remainder, on the table's device."""
    n, b = table.shape[0], block.shape[0]
    full = n // b
    if full:
        table[:full * b].unflatten(0, (full, b)).copy_(block.unsqueeze(0).expand((full,) + tuple(block.shape)))
    if n % b:
        table[full * b:].copy_(block[:n % b])


class TallCase:
    """A table of ``n_rows`` rows of ``ld`` elements (``itemsize`` bytes each) whose row starts straddle ``marks``.

    ``rows``   the kept rows, ascending: the mark rows, ``n_extra`` seeded random rows, the neighbours of every mark row; every
               fourth of the random rows and the two rows either side of each mark row stay BALLAST (``is_ballast``), the others
               are LIVE: seeded standard-normal float32 data.
    ``values`` float32 [len(rows), width]: what the table holds in those rows (the twin table, as it is)."""

    def __init__(self, marks, ld, width=None, itemsize=4, seed=0, n_extra=240, margin_rows=160, ballast_rows=3001, more_pitches=()):
        """``more_pitches``: row pitches in bytes of OTHER operands with the same rows (an ``out`` with another leading dimension,
        an output of another element size): their mark rows are mark rows of this case too, and n_rows reaches beyond the marks
        for every pitch."""
        self.marks, self.ld, self.width, self.itemsize = tuple(marks), int(ld), int(width or ld), itemsize
        self.pitch = self.ld * itemsize
        self.roles_by_pitch = {p: tall_rows(marks, p, margin_rows) for p in (self.pitch,) + tuple(more_pitches)}
        self.n_rows = max(n for n, _ in self.roles_by_pitch.values())
        self.roles_by_pitch = {p: dict(ro, last=self.n_rows - 1) for p, (_, ro) in self.roles_by_pitch.items()}
        self.roles = self.roles_by_pitch[self.pitch]
        self.ballast_rows = min(ballast_rows, self.n_rows)
        rng = np.random.default_rng([seed, self.ld, len(marks)])
        mark_rows = np.unique(np.array([r for ro in self.roles_by_pitch.values() for r in ro.values()], np.int64))
        extra = rng.choice(self.n_rows, size=min(n_extra, self.n_rows), replace=False)
        near = np.concatenate([mark_rows - 2, mark_rows + 2])
        near = near[(near >= 0) & (near < self.n_rows)]
        near = np.setdiff1d(near, mark_rows)
        self.mark_rows = mark_rows
        self.rows = np.unique(np.concatenate([mark_rows, extra, near]))
        ballast = np.union1d(near, np.setdiff1d(extra, mark_rows)[::4])
        self.is_ballast = np.isin(self.rows, ballast)
        self.values = rng.standard_normal((len(self.rows), self.width)).astype(np.float32)
        self.values[self.is_ballast] = ballast_values(self.rows[self.is_ballast] % self.ballast_rows, self.width)

    @property
    def live(self):
        return self.rows[~self.is_ballast]

    def twin_ids(self, ids):
        """The monotone remap: table row -> row of the twin table (``values``)."""
        ids = np.asarray(ids, np.int64)
        pos = np.searchsorted(self.rows, ids)
        assert np.array_equal(self.rows[pos], ids), "not a kept row"
        return pos

    def offsets(self, ids=None):
        """Byte offsets of the starts of rows ``ids`` (default: the kept rows) from the table's base."""
        return np.asarray(self.rows if ids is None else ids, np.int64) * self.pitch

    def check_straddle(self, table=None):
        """The promises of the mark rows, from the rows' byte ranges -- for the pitch of the built operand ``table`` (which must
        be one of the case's pitches), and from ITS shape and strides, when one is given; for the case's own pitch otherwise."""
        p = self.pitch if table is None else table.stride(0) * table.element_size()
        ro = self.roles_by_pitch[p]
        for m in self.marks:
            b, a, n = ro[("below", m)], ro[("at", m)], ro[("after", m)]
            assert (b + 1) * p <= m < (b + 2) * p and a * p <= m < (a + 1) * p and n * p > m and n == a + 1 == b + 2
            assert ((b + 1) * p == m) == (m % p == 0) == (a * p == m)
            assert b in self.live and a in self.live and n in self.live
        assert (self.n_rows - 1) * p > max(self.marks) and 0 in self.live and self.n_rows - 1 in self.live
        if table is not None:
            assert table.shape[0] == self.n_rows and (table.shape[0] - 1) * table.stride(0) * table.element_size() > max(self.marks)

    def build(self, device, dtype=torch.float32, pad=float("nan")):
        """-> (view [n_rows, width] with row stride ld, buffer [n_rows, ld]): ballast everywhere, the kept rows' values written
        over it, the columns beyond ``width`` (if any) set to ``pad``."""
        buf = torch.empty((self.n_rows, self.ld), dtype=dtype, device=device)
        block = torch.from_numpy(ballast_values(np.arange(self.ballast_rows), self.ld)).to(device=device, dtype=dtype)
        fill_periodic(buf, block)
        if self.ld > self.width:
            buf[:, self.width:] = pad
        view = buf[:, :self.width]
        view[torch.from_numpy(self.rows).to(device)] = torch.from_numpy(self.values).to(device=device, dtype=dtype)
        return view, buf

    def twin(self, device, dtype=torch.float32):
        return torch.from_numpy(self.values).to(device=device, dtype=dtype)

    def samples(self, k=3):
        """Rows NOT kept, next to every mark and at both ends: ballast whose outputs are sampled."""
        out = []
        for r in self.mark_rows:
            out.extend(range(max(int(r) - k - 2, 0), min(int(r) + k + 3, self.n_rows)))
        return np.setdiff1d(np.array(out, np.int64), self.rows)


def out_buffer(n_rows, ld, col0, width, device, guard_rows=2):
    """A SENTINEL-filled int32 buffer [(n_rows + 2 guard_rows), ld] seen as float32 -> (view of rows guard_rows .., columns
    col0 .. col0 + width, buffer): the ``out=`` of a call and the guard regions around it (layer_truth.out_operand, tall)."""
    buf = torch.full((n_rows + 2 * guard_rows, ld), SENTINEL, dtype=torch.int32, device=device).view(torch.float32)
    return buf[guard_rows:guard_rows + n_rows, col0:col0 + width], buf


def guards_intact(buf, view):
    """No word of ``buf`` outside ``view`` changed and no word inside it still holds SENTINEL (reductions on the buffer's device)."""
    words = buf.view(torch.int32)
    off = (view.data_ptr() - buf.data_ptr()) // 4
    r0, c0 = off // buf.stride(0), off % buf.stride(0)
    r1, c1 = r0 + view.shape[0], c0 + view.shape[1]
    outside = [words[:r0], words[r1:], words[r0:r1, :c0], words[r0:r1, c1:]]
    clean = all(bool((w == SENTINEL).all()) for w in outside if w.numel())
    return clean and not bool((words[r0:r1, c0:c1] == SENTINEL).any())


ROW_LENGTHS = [1, 31, 32, 33, 63, 64, 65, 129]   # layer_truth.LAYER_ROWS without the empty row and the hub


def tall_graph(case, seed=1, n_more=24):
    """A directed weighted graph over the table's rows in which only kept rows have entries and every entry is a kept row:
    each mark row and ``n_more`` further live rows hold ROW_LENGTHS[i % 8] entries drawn from the kept rows (mark rows first,
    so every mark row is READ as well as written), fractional float32 values in (0.05, 3).
    -> dict(rows int64 [R] ascending, indptr int64 [R + 1], col int64 [nnz] (table ids, sorted per row), val float32 [nnz])."""
    rng = np.random.default_rng([seed, case.ld])
    others = np.setdiff1d(case.live, case.mark_rows)
    rows = np.sort(np.concatenate([case.mark_rows, rng.choice(others, size=min(n_more, len(others)), replace=False)]))
    cols, indptr = [], [0]
    for i, _ in enumerate(rows):
        ln = min(ROW_LENGTHS[i % len(ROW_LENGTHS)], len(case.rows))
        k = min(ln, len(case.mark_rows), 4)
        head = rng.choice(case.mark_rows, size=k, replace=False)
        rest = rng.choice(np.setdiff1d(case.rows, head), size=ln - k, replace=False)
        cols.append(np.sort(np.concatenate([head, rest])))
        indptr.append(indptr[-1] + ln)
    col = np.concatenate(cols).astype(np.int64)
    val = rng.uniform(0.051, 2.999, len(col)).astype(np.float32)
    return dict(rows=rows, indptr=np.array(indptr, np.int64), col=col, val=val)


def tall_graph_device(case, g, device):
    """(rowptr int64 [n_rows + 1], col int32, val float32) of ``tall_graph`` over all n_rows nodes; the row pointer is built on
    the device from the live rows' lengths (nothing of the table's length is generated on the host)."""
    deg = torch.zeros(case.n_rows + 1, dtype=torch.int64, device=device)
    deg[torch.from_numpy(g["rows"] + 1).to(device)] = torch.from_numpy(np.diff(g["indptr"])).to(device)
    rowptr = torch.cumsum(deg, 0)
    return rowptr, torch.from_numpy(g["col"].astype(np.int32)).to(device), torch.from_numpy(g["val"]).to(device)


def tall_graph_twin(case, g):
    """The same graph over the kept rows alone -> scipy CSR float64 [K, K] (K = len(case.rows)), ids remapped by twin_ids."""
    k = len(case.rows)
    indptr = np.zeros(k + 1, np.int64)
    indptr[case.twin_ids(g["rows"]) + 1] = np.diff(g["indptr"])
    np.cumsum(indptr, out=indptr)
    A = ssp.csr_matrix((g["val"].astype(np.float64), case.twin_ids(g["col"]).astype(np.int32), indptr), shape=(k, k))
    assert A.has_sorted_indices
    return A


# ====================================================================================================================
# long entry arrays
# ====================================================================================================================
def ballast_entry_values(L):
    """The stored values of a ballast row's L entries: multiples of 1/4 in [0.25, 1.25]."""
    return ((np.arange(L) % 5 + 1) * 0.25).astype(np.float32)


class LongCSR:
    """A directed pattern over ``n`` nodes whose entry array crosses the entry indices mark // entry_bytes.

    Rows, in storage order: ballast, live set 0, ballast, live set 1, ..., ballast, the last live set (it ends the arrays); the
    rows after that are empty.  Ballast rows hold the run 0 .. L - 1 (a group's last row the remainder of the run), so a whole
    ballast region is the ramp 0 .. L - 1 over and over.  A live set holds one row of every length of ``lens``, random sorted
    neighbourhoods drawn from a pool of ids, values uniform in (0.05, 3).  Set i (i < len(marks)) is placed by ``kinds[i]``:
    'edge': row ``b`` of the set ENDS exactly at the mark's entry index and row b + 1 STARTS there; 'span': row b holds it
    strictly inside.  ``phase`` swaps the kinds, so two builds give every mark both.

    Host data: ``rowptr`` (int64 [n + 1]); ``live`` = [(row id, first entry, ids int32, values float32)] in storage order;
    ``ballast`` = [(first row, first entry, entries)] per region."""

    def __init__(self, marks, lens, L, b, phase=0, entry_bytes=4, seed=0, tail_rows=2, pool=None):
        self.marks, self.lens, self.L, self.b = tuple(sorted(marks)), list(lens), int(L), int(b)
        self.entry_bytes = entry_bytes
        assert 0 <= b < len(lens) - 1 and lens[b] >= 2
        T = sum(lens)
        self.positions = [m // entry_bytes for m in self.marks]
        self.kinds = [("edge", "span")[(i + phase) % 2] for i in range(len(self.marks))]
        starts = []
        for p, kind in zip(self.positions, self.kinds):
            pre = sum(lens[:b + 1]) if kind == "edge" else sum(lens[:b]) + lens[b] // 2
            starts.append(p - pre)
        starts.append(starts[-1] + T + tail_rows * L + L // 3)                  # the set that ends the arrays
        self.nnz = starts[-1] + T
        rng = np.random.default_rng([seed, L, len(lens)])
        # rows
        ptr, self.live, self.ballast, self.set_rows = [0], [], [], []
        cursor = 0
        for s in starts:
            assert s >= cursor, "the live sets overlap: marks too close for these lengths"
            full, rem = divmod(s - cursor, L)
            if s > cursor:
                self.ballast.append((len(ptr) - 1, cursor, s - cursor))
            ptr.extend(cursor + L * (i + 1) for i in range(full))
            if rem:
                ptr.append(s)
            first = len(ptr) - 1
            for ln in lens:
                ptr.append(ptr[-1] + ln)
            self.set_rows.append(np.arange(first, first + len(lens)))
            cursor = s + T
        n_used = len(ptr) - 1
        self.n = max(self.L, n_used + 8)
        self.n_used = n_used
        self.rowptr = np.full(self.n + 1, self.nnz, np.int64)
        self.rowptr[:len(ptr)] = ptr
        pool_size = min(self.n, max(2 * max(lens), 64)) if pool is None else pool
        # (a quarter of the pool are STORED rows: entries whose column has a row sum -- gcn_norm's non-zero terms)
        ids = np.unique(np.concatenate([rng.choice(self.n, size=pool_size, replace=False),
                                        rng.choice(n_used, size=min(n_used, pool_size // 4), replace=False), [0, self.n - 1]]))
        for rows in self.set_rows:
            for r, ln in zip(rows, lens):
                c = np.sort(rng.choice(ids, size=ln, replace=False)).astype(np.int32)
                self.live.append((int(r), int(self.rowptr[r]), c, rng.uniform(0.051, 2.999, ln).astype(np.float32)))
        self.live_rows = np.array([r for r, _, _, _ in self.live], np.int64)
        self.ballast_rows = np.setdiff1d(np.arange(n_used), self.live_rows)
        self.full_ballast_rows = self.ballast_rows[np.diff(self.rowptr)[self.ballast_rows] == L]

    # ------------------------------------------------------------------ promises
    def check_straddle(self, col=None):
        """Every mark's entry index lies in a live row as its kind says; the arrays end in a live row -- and, given the built
        ``col``, its byte size is beyond every mark."""
        rp = self.rowptr
        for i, (p, kind) in enumerate(zip(self.positions, self.kinds)):
            rows = self.set_rows[i]
            rb = rows[self.b]
            if kind == "edge":
                assert rp[rb + 1] == p == rp[rows[self.b + 1]] and rp[rb] < p < rp[rb + 2]
            else:
                assert rp[rb] < p < rp[rb + 1]
            assert rb in self.live_rows
        assert rp[self.set_rows[-1][-1] + 1] == self.nnz == rp[-1]
        if col is not None:
            assert col.numel() == self.nnz and col.numel() * col.element_size() > max(self.marks)
            assert col.element_size() == self.entry_bytes

    # ------------------------------------------------------------------ device arrays
    def _fill(self, out, ramp, live_index):
        for _, e0, cnt in self.ballast:
            fill_periodic(out[e0:e0 + cnt], ramp)
        for rows in self.set_rows:
            parts = [self.live[i][live_index] for i in range(len(self.live)) if self.live[i][0] in rows]
            e0 = int(self.rowptr[rows[0]])
            blob = torch.from_numpy(np.concatenate(parts)).to(out.device)
            out[e0:e0 + blob.numel()].copy_(blob)

    def build(self, device, weighted=True):
        """-> (rowptr, col, val | None) on ``device``: the ballast regions by broadcast copies of one ramp of L entries."""
        col = torch.empty(self.nnz, dtype=torch.int32, device=device)
        self._fill(col, torch.arange(self.L, dtype=torch.int32, device=device), 2)
        val = None
        if weighted:
            val = torch.empty(self.nnz, dtype=torch.float32, device=device)
            self._fill(val, torch.from_numpy(ballast_entry_values(self.L)).to(device), 3)
        return torch.from_numpy(self.rowptr).to(device), col, val

    # ------------------------------------------------------------------ the twin
    def kept_ballast(self):
        """The ballast rows the twin keeps: the first full one, the full one nearest below every live set (the one below the
        top mark's set ends just under it), the last full one (beyond every mark), a remainder row."""
        keep = [int(self.full_ballast_rows[0]), int(self.full_ballast_rows[-1])] if len(self.full_ballast_rows) else []
        for rows in self.set_rows:
            below = self.full_ballast_rows[self.full_ballast_rows < rows[0]]
            if len(below):
                keep.append(int(below[-1]))
        part = np.setdiff1d(self.ballast_rows, self.full_ballast_rows)
        if len(part):
            keep.append(int(part[0]))
        return np.unique(np.array(keep, np.int64))

    def pair_ballast(self):
        """The ballast rows the pair lists use: the first, the full one just below the top mark, the last, a remainder row."""
        top = self.set_rows[len(self.marks) - 1][0]
        keep = [self.full_ballast_rows[0], self.full_ballast_rows[self.full_ballast_rows < top][-1], self.full_ballast_rows[-1]]
        part = np.setdiff1d(self.ballast_rows, self.full_ballast_rows)
        if len(part):
            keep.append(part[0])
        return np.unique(np.array(keep, np.int64))

    def row(self, r):
        """(ids int32, values float32) of stored row ``r``, live or ballast, from the host data."""
        hit = np.flatnonzero(self.live_rows == r)
        if len(hit):
            return self.live[int(hit[0])][2], self.live[int(hit[0])][3]
        ln = int(self.rowptr[r + 1] - self.rowptr[r])
        return np.arange(ln, dtype=np.int32), ballast_entry_values(self.L)[:ln]

    def twin(self, extra_rows=None):
        """scipy CSR float32 [n, n]: the live rows and ``kept_ballast()`` (plus ``extra_rows``) at their own row ids -- the id map
        is the identity, which is monotone -- and every other row empty: the same rows at entry offsets of a few MB at most."""
        keep = np.union1d(self.live_rows, self.kept_ballast())
        if extra_rows is not None:
            keep = np.union1d(keep, np.asarray(extra_rows, np.int64))
        indptr = np.zeros(self.n + 1, np.int64)
        parts = [self.row(int(r)) for r in keep]
        indptr[keep + 1] = [len(c) for c, _ in parts]
        np.cumsum(indptr, out=indptr)
        A = ssp.csr_matrix((np.concatenate([v for _, v in parts]), np.concatenate([c for c, _ in parts]), indptr),
                           shape=(self.n, self.n))
        A.has_sorted_indices = True
        return A, keep

    # ------------------------------------------------------------------ whole-array truths from the host data
    def row_sums(self, weighted=True):
        """float64 [n]: the sum of every row's stored values (unit: its length)."""
        if not weighted:
            return np.diff(self.rowptr).astype(np.float64)
        pre = np.concatenate([[0.0], np.cumsum(ballast_entry_values(self.L).astype(np.float64))])
        s = pre[np.diff(self.rowptr)[:self.n_used].clip(max=self.L)]
        s = np.concatenate([s, np.zeros(self.n - self.n_used)])
        for r, _, _, v in self.live:
            s[r] = v.astype(np.float64).sum()
        return s

    def col_sums(self, weighted=True):
        """(float64 [n] column sums, float64 [n] sums of the absolute live terms, int64 [n] stored entries per column): ballast
        from the rows' lengths (a row of l entries holds the columns below l), live entries added one by one."""
        deg = np.diff(self.rowptr)[self.ballast_rows]
        cnt = np.zeros(self.n + 1, np.int64)
        np.add.at(cnt, 0, len(deg))
        np.add.at(cnt, deg, -1)
        cnt = np.cumsum(cnt)[:self.n]
        vb = np.ones(self.n)
        if weighted:
            vb[:self.L] = ballast_entry_values(self.L)
        s, a, k = cnt * vb, np.zeros(self.n), cnt.copy()
        for _, _, c, v in self.live:
            t = v.astype(np.float64) if weighted else np.ones(len(c))
            np.add.at(s, c, t); np.add.at(a, c, np.abs(t)); np.add.at(k, c, 1)
        return s, a, k

    def entry(self, k):
        """(row, column id, float32 value) of stored entries ``k`` (an int64 array), from the host data."""
        k = np.asarray(k, np.int64)
        row = np.searchsorted(self.rowptr, k, side="right") - 1
        col = k - self.rowptr[row]                                          # a ballast row holds the ramp
        val = ((col % 5 + 1) * 0.25).astype(np.float32)
        for r, s0, c, v in self.live:
            m = row == r
            if m.any():
                col[m], val[m] = c[k[m] - s0], v[k[m] - s0]
        return row, col, val

    def sample_entries(self, k=4):
        """Entry indices next to every mark, at both ends of the arrays, and at the head and end of the ballast row below
        every live set (heads: columns that are stored rows, whose gcn_norm terms are not zero)."""
        out = [np.arange(0, min(3 * k, self.nnz)), np.arange(max(self.nnz - k, 0), self.nnz)]
        for p in self.positions:
            out.append(np.arange(max(p - k, 0), min(p + k, self.nnz)))
        for rows in self.set_rows:
            s = int(self.rowptr[rows[0]])
            out.append(np.arange(max(s - k, 0), s))
            below = self.full_ballast_rows[self.full_ballast_rows < rows[0]]
            if len(below):
                out.append(int(self.rowptr[below[-1]]) + np.arange(0, min(3 * k, self.L)))
        return np.unique(np.concatenate(out))


def gcn_norm_at(case, k, weighted=True):
    """(truth float64, bound) of eps_gcn_norm's output at entries ``k``: layer_truth.gcn_norm / gcn_norm_bound restated per
    entry from the host data (val / sqrt(s_r s_c), 0 where a sum is 0; ((deg_r + deg_c) / 2 U + 1e-6) |truth|)."""
    row, col, val = case.entry(k)
    s = case.row_sums(weighted)
    v = val.astype(np.float64) if weighted else np.ones(len(row))
    den = s[row] * s[col]
    truth = np.where(den != 0, v / np.sqrt(np.where(den != 0, den, 1.0)), 0.0)
    deg = np.diff(case.rowptr).astype(np.float64)
    return truth, ((deg[row] + deg[col]) / 2 * 2.0 ** -24 + 1e-6) * np.abs(truth)


def pair_lists(case):
    """Pairs over the live rows and a few ballast rows -> (u, v) int32, sorted by v (runs of equal v: the column-run kernel's
    order): every live row against every row of its set and of the next set; the two rows at the set's mark (rows b, b + 1) against
    each of ``pair_ballast()``, both ways round; two ballast rows against each other."""
    kb = case.pair_ballast()
    u, v = [], []
    for i, rows in enumerate(case.set_rows):
        other = case.set_rows[(i + 1) % len(case.set_rows)]
        for a in rows:
            for bb in np.concatenate([rows, other]):
                u.append(a); v.append(bb)
        for a in rows[case.b:case.b + 2]:
            for bb in kb:
                u.extend([a, bb]); v.extend([bb, a])
    if len(kb) > 1:
        u.extend([kb[0], kb[-1]]); v.extend([kb[-1], kb[0]])
    u, v = np.array(u, np.int32), np.array(v, np.int32)
    o = np.argsort(v, kind="stable")
    return u[o], v[o]


def gammas_truth(case, ptr, w):
    """local_community_truth.gammas restated from the host data: for member x of a segment, the stored entries of row x among the
    OTHER members.  A ballast (or empty) row of l entries holds the ids below l: the members below l, less x itself if x < l; a
    live row is intersected with the segment.  (The host test holds it to local_community_truth.gammas on a whole small graph.)"""
    ptr, w = np.asarray(ptr, np.int64), np.asarray(w, np.int64)
    deg = np.diff(case.rowptr)
    out = np.zeros(len(w), np.int64)
    for b in range(len(ptr) - 1):
        seg = w[ptr[b]:ptr[b + 1]]
        if len(seg) == 0:
            continue
        ln = deg[seg]
        g = np.searchsorted(seg, ln, side="left") - (seg < ln)
        for j in np.flatnonzero(np.isin(seg, case.live_rows)):
            ids = case.row(int(seg[j]))[0]
            g[j] = np.isin(ids, seg).sum() - int(seg[j] in ids)
        out[ptr[b]:ptr[b + 1]] = g
    return out


def pair_truth(case, weighted, node_w, u, v):
    """pair_score_truth.scores for the pairs of ``pair_lists``: the pairs of two live rows by pair_score_truth.scores itself (on
    the live rows of the twin); a pair with a ballast row -- the ramp 0 .. l - 1, of up to L entries -- by the same definition
    restated per pair (products and sums in extended precision, rounded to float64 once), which the host test holds to
    pair_score_truth.scores on a whole small graph."""
    u, v = np.asarray(u, np.int64), np.asarray(v, np.int64)
    w = np.asarray(node_w)
    keys = ("count", "cn", "ws", "abs_cn", "abs")
    out = {k: np.zeros(len(u), np.int64 if k == "count" else np.float64) for k in keys}
    live = np.isin(u, case.live_rows) & np.isin(v, case.live_rows)
    indptr = np.zeros(case.n + 1, np.int64)
    indptr[case.live_rows + 1] = [len(c) for _, _, c, _ in case.live]
    np.cumsum(indptr, out=indptr)
    order = np.argsort(case.live_rows)
    data = np.concatenate([case.live[i][3] for i in order]) if weighted else np.ones(int(indptr[-1]), np.float32)
    A = ssp.csr_matrix((data, np.concatenate([case.live[i][2] for i in order]), indptr), shape=(case.n, case.n))
    A.has_sorted_indices = True
    t = pt.scores(A, w, u[live], v[live])
    for k in keys:
        out[k][live] = t[k]
    is_b = lambda r: r not in case.live_rows                                                      # noqa: E731
    for i in np.flatnonzero(~live):
        (ca, va), (cb, vb) = case.row(int(u[i])), case.row(int(v[i]))
        if is_b(v[i]):                                                      # b holds the ramp: the common ids are those of a below its length
            m = ca < len(cb)
            ids, xa, xb = ca[m], va[m], vb[ca[m]]
        else:
            m = cb < len(ca)
            ids, xa, xb = cb[m], va[cb[m]], vb[m]
        one = np.ones(len(ids), pt.WIDE)
        t_cn = (xa.astype(pt.WIDE) * xb.astype(pt.WIDE)) if weighted else one
        t_ws = t_cn * w[ids].astype(pt.WIDE)
        out["count"][i] = len(ids)
        out["cn"][i], out["ws"][i] = np.float64(t_cn.sum()), np.float64(t_ws.sum())
        out["abs_cn"][i], out["abs"][i] = np.float64(np.abs(t_cn).sum()), np.float64(np.abs(t_ws).sum())
    return out
