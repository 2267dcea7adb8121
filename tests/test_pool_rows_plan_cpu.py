"""CPU-only: which pooled rows a step of a pool call serves, as runs of armed / raw rows (csrc/ifa_pool_rows_plan.h, through
ifa_pool_rows_plan) against runs written by hand, and a sweep over every armed / raw pattern of up to 8 rows in up to 3 chunks."""
import ctypes as C
import itertools

import pytest

import inferflow_amd as ia


def plan(rows_sel, adj, cursor, chunk0, n_rows):
    """-> ([(ja, jb, armed)], cursor behind the step)"""
    n = len(rows_sel)
    rs = (C.c_int * max(n, 1))(*rows_sel)
    ad = None if adj is None else (C.c_int * max(n, 1))(*adj)
    runs = (C.c_int * (3 * max(n, 1)))()
    n_runs, cur = C.c_int(-1), C.c_int(-1)
    ia.check(ia.lib().ifa_pool_rows_plan(rs, ad, n, cursor, chunk0, n_rows, runs, max(n, 1), C.byref(n_runs), C.byref(cur)))
    return [tuple(runs[3 * i:3 * i + 3]) for i in range(n_runs.value)], cur.value


def call(rows_sel, adj, chunks):
    """the steps of a call taken as `chunks` = [(chunk0, n_rows)]: the runs of each step"""
    cur, out = 0, []
    for c0, nr in chunks:
        runs, cur = plan(rows_sel, adj, cur, c0, nr)
        out.append(runs)
    return out, cur


# (name, rows_sel, adj, [(chunk0, n_rows)], the runs of each step, the cursor behind the last)
TABLE = [
    ("one row", [0], [3], [(0, 1)], [[(0, 1, 1)]], 1),
    ("one raw row of a larger step", [2], None, [(0, 4)], [[(0, 1, 0)]], 1),
    ("all raw, no adjust armed", [0, 1, 2, 3], None, [(0, 4)], [[(0, 4, 0)]], 4),
    ("all raw, slots given", [0, 2, 5], [-1, -1, -1], [(0, 6)], [[(0, 3, 0)]], 3),
    ("all armed", [0, 1, 2, 3], [4, 0, 2, 9], [(0, 4)], [[(0, 4, 1)]], 4),
    ("alternating", [0, 1, 2, 3, 4], [1, -1, 0, -1, 2], [(0, 5)], [[(0, 1, 1), (1, 2, 0), (2, 3, 1), (3, 4, 0), (4, 5, 1)]], 5),
    ("rows 0 and 2 of 3, only row 2 armed", [0, 2], [-1, 2], [(0, 3)], [[(0, 1, 0), (1, 2, 1)]], 2),
    # 20 rows as two steps of 10: the armed run of pooled rows 1..3 (rows 8, 9, 10) straddles the border and is cut there
    ("a run across the chunk border", [3, 8, 9, 10, 15], [-1, 5, 5, 5, -1], [(0, 10), (10, 10)],
     [[(0, 1, 0), (1, 3, 1)], [(3, 4, 1), (4, 5, 0)]], 5),
    ("a chunk without a pooled row", [1, 17], [0, 0], [(0, 6), (6, 6), (12, 6)], [[(0, 1, 1)], [], [(1, 2, 1)]], 2),
    ("pooled rows in the last chunk only", [16, 17, 31], None, [(0, 16), (16, 16)], [[], [(0, 3, 0)]], 3),
]


@pytest.mark.parametrize("name,rows_sel,adj,chunks,want,want_cur", TABLE, ids=[t[0] for t in TABLE])
def test_runs_written_by_hand(name, rows_sel, adj, chunks, want, want_cur):
    got, cur = call(rows_sel, adj, chunks)
    assert got == want and cur == want_cur, (name, got, cur)


def test_cursor_already_at_n_sel():
    assert plan([0, 1, 2], [1, 1, 1], 3, 0, 3) == ([], 3)
    assert plan([0, 1, 2], None, 3, 16, 16) == ([], 3)
    assert plan([], None, 0, 0, 4) == ([], 0)


def test_the_device_fed_case_is_one_chunk_from_cursor_zero():
    assert plan([0, 2, 3], [-1, 2, 3], 0, 0, 4) == ([(0, 1, 0), (1, 3, 1)], 3)


def test_bad_arguments_are_refused():
    L = ia.lib()
    n_runs, cur = C.c_int(), C.c_int()
    rs, runs = (C.c_int * 2)(1, 1), (C.c_int * 6)()
    assert L.ifa_pool_rows_plan(rs, None, 2, 0, 0, 4, runs, 2, C.byref(n_runs), C.byref(cur)) != 0       # not ascending
    rs = (C.c_int * 2)(0, 1)
    assert L.ifa_pool_rows_plan(rs, None, 2, 3, 0, 4, runs, 2, C.byref(n_runs), C.byref(cur)) != 0       # cursor past n_sel
    assert L.ifa_pool_rows_plan(rs, (C.c_int * 2)(1, -1), 2, 0, 0, 4, runs, 1, C.byref(n_runs), C.byref(cur)) != 0      # no room for 2 runs
    assert L.ifa_pool_rows_plan(rs, None, 2, 0, 0, 4, runs, 2, None, C.byref(cur)) != 0


def test_sweep_every_pattern_of_up_to_8_rows_in_up_to_3_chunks():
    """every pooled row is served exactly once, in order; every run is uniform, and maximal within its chunk.  Up to 6 rows: every
    row not pooled / raw / armed; 7 and 8 rows: every row pooled, raw or armed (the rows a step does not pool are covered above)"""
    for n in range(1, 9):
        cuts = [()] + [(a,) for a in range(1, n)] + [(a, b) for a in range(1, n) for b in range(a + 1, n)]
        for pooled in range(1, 1 << n) if n <= 6 else [(1 << n) - 1]:
            rows_sel = [r for r in range(n) if pooled >> r & 1]
            for armed in itertools.product((0, 1), repeat=len(rows_sel)):
                adj = [5 if a else -1 for a in armed]
                for cut in cuts:
                    edges = (0,) + cut + (n,)
                    chunks = [(edges[i], edges[i + 1] - edges[i]) for i in range(len(edges) - 1)]
                    steps, cur = call(rows_sel, adj, chunks)
                    assert cur == len(rows_sel)
                    served = []
                    for (c0, nr), runs in zip(chunks, steps):
                        for i, (ja, jb, a) in enumerate(runs):
                            assert ja < jb and all(armed[j] == a for j in range(ja, jb)), (rows_sel, adj, chunks, runs)
                            assert all(c0 <= rows_sel[j] < c0 + nr for j in range(ja, jb)), (rows_sel, chunks, runs)
                            if i:      # maximal: the run before it in this chunk ends here and differs
                                assert runs[i - 1][1] == ja and runs[i - 1][2] != a, (rows_sel, adj, chunks, runs)
                            served += list(range(ja, jb))
                    assert served == list(range(len(rows_sel))), (rows_sel, adj, chunks, steps)
