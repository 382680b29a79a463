"""Sparse matrix-vector products over a prime field in Python integers: what libmsm_frmat.so (include/msm_frmat.h) computes.  A matrix is CSR --
row_ptr (rows + 1), col_idx and values (nnz each) --; within a row the columns come in any order and may repeat, repeated entries add."""


def matvec(rows, cols, row_ptr, col_idx, values, x, r, transpose=False):
    """y = M x (len rows), or with transpose M^T x (len cols), mod r"""
    assert len(row_ptr) == rows + 1 and len(col_idx) == len(values) == row_ptr[rows] and len(x) == (rows if transpose else cols)
    y = [0] * (cols if transpose else rows)
    for i in range(rows):
        for e in range(row_ptr[i], row_ptr[i + 1]):
            if transpose:
                y[col_idx[e]] = (y[col_idx[e]] + values[e] * x[i]) % r
            else:
                y[i] = (y[i] + values[e] * x[col_idx[e]]) % r
    return y


def transpose_csr(rows, cols, row_ptr, col_idx, values):
    """-> (t_ptr, t_idx, t_values): the CSR arrays of M^T (cols x rows); within a row of M^T the entries keep the order they have in M"""
    buckets = [[] for _ in range(cols)]
    for i in range(rows):
        for e in range(row_ptr[i], row_ptr[i + 1]):
            buckets[col_idx[e]].append((i, values[e]))
    t_ptr = [0]
    for b in buckets:
        t_ptr.append(t_ptr[-1] + len(b))
    return t_ptr, [i for b in buckets for i, _ in b], [v for b in buckets for _, v in b]


def levels(row_ptr, tile):
    """how many passes the product takes (csrc/frmat_plan.h): the tiles of `tile` entries, then the partial sums of the rows that cross tiles,
    and so on while there are any; 0 without entries.  The launches are one more: the fill of y."""
    row_of = [i for i in range(len(row_ptr) - 1) for _ in range(row_ptr[i], row_ptr[i + 1])]
    count = 0
    while row_of:
        count += 1
        nxt, n = [], len(row_of)
        for s in range(0, n, tile):
            e = min(n, s + tile)
            head = s > 0 and row_of[s - 1] == row_of[s]
            tail = e < n and row_of[e] == row_of[e - 1]
            if head:
                nxt.append(row_of[s])
            if tail and not (head and row_of[s] == row_of[e - 1]):
                nxt.append(row_of[e - 1])
        row_of = nxt
    return count


def mont(vals, r, back=False):
    """plain values -> a * 2^256 mod r (back=True: the other way)"""
    f = pow(2, 256, r)
    if back:
        f = pow(f, r - 2, r)
    return [v * f % r for v in vals]


def to_bytes(vals):
    return b"".join(int(v).to_bytes(32, "little") for v in vals)


def from_bytes(b):
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


# ---- the shapes both the host test and the GPU test run: name -> (tile, rows, cols, row_ptr, col_idx); values are the caller's -----------------------
def _ptr(lengths):
    out = [0]
    for n in lengths:
        out.append(out[-1] + n)
    return out


def shape(name, rnd):
    """(tile, rows, cols, row_ptr, col_idx) of a named shape; rnd: a random.Random for the columns"""
    def cols_for(ptr, cols):
        return [rnd.randrange(cols) for _ in range(ptr[-1])]

    if name == "1x1 empty":
        return 1024, 1, 1, [0, 0], []
    if name == "1x1 one entry":
        return 1024, 1, 1, [0, 1], [0]
    if name == "1030 single-entry rows":  # two tiles
        return 1024, 1030, 37, _ptr([1] * 1030), [rnd.randrange(37) for _ in range(1030)]
    if name == "one row of 2050":  # a row over three tiles, short rows around it
        ptr = _ptr([2, 0, 1, 2050, 3, 1])
        return 1024, 6, 61, ptr, cols_for(ptr, 61)
    if name == "9x7 with empty rows":  # leading, trailing and consecutive empty rows
        ptr = _ptr([0, 0, 3, 0, 0, 2, 6, 0, 0])
        return 4, 9, 7, ptr, cols_for(ptr, 7)
    if name == "row ends on a tile boundary":
        ptr = _ptr([3, 1, 4, 2, 6, 1])
        return 4, 6, 5, ptr, cols_for(ptr, 5)
    if name == "one row of 70":  # 70 -> 18 -> 5 -> 2 partials: four levels
        return 4, 1, 9, [0, 70], [rnd.randrange(9) for _ in range(70)]
    if name == "all entries in one row":
        ptr = _ptr([0, 0, 23, 0, 0])
        return 4, 5, 6, ptr, cols_for(ptr, 6)
    if name in ("random tile 2", "random tile 8"):  # repeated and unsorted columns
        tile = int(name.split()[-1])
        lengths = [rnd.choice((0, 1, 1, 2, 3, 5, 9, 17)) for _ in range(13)]
        ptr = _ptr(lengths)
        return tile, 13, 5, ptr, cols_for(ptr, 5)
    raise KeyError(name)


SMALL_SHAPES = ("9x7 with empty rows", "row ends on a tile boundary", "one row of 70", "all entries in one row", "random tile 2", "random tile 8")
DESIGN_SHAPES = ("1x1 empty", "1x1 one entry", "1030 single-entry rows", "one row of 2050")
# the passes of every shape, worked out by hand from the tile and the row lengths (the fill of y is one launch more):
#   no entry: none.  One tile, or rows that end with their tiles: 1.  2050 entries of one row over tiles of 1024 (with two entries before it):
#   three tiles hold a part of it, their three partials are one tile of the second pass: 2.  70 entries over tiles of 4: 18 partials, then 5,
#   then 2, then one tile: 4.  23 entries of one row over tiles of 4: 6 partials, then 2, then one tile: 3.
LEVELS = {"1x1 empty": 0, "1x1 one entry": 1, "1030 single-entry rows": 1, "one row of 2050": 2, "9x7 with empty rows": 2, "row ends on a tile boundary": 2,
          "one row of 70": 4, "all entries in one row": 3}
