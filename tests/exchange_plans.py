"""The exchange plan of csrc/ctg_plan.h (exchange_plan, seg_of) restated in
Python integers, and the count matrices the CPU tests sweep
(tests/test_plan.py through tools/plan_check.cpp, tests/test_dist_cpu.py
against dist.segment_words).  Test infrastructure only.

A count matrix is counts[src][dst] = (rows, nodes) of src's table that dst
owns.  A rank's send table has one segment per destination with rows or
nodes, in rank order, the rank itself left out; its receive table the same
over the sources."""
from __future__ import annotations

ROW = 28          # CTG_MGPU_ROW_WORDS
MAX_WORLD = 32    # CTG_MGPU_MAX_WORLD
LIMIT = 1 << 32   # the merge's row indices are u32


def flat(counts):
    return ' '.join('%d %d' % tuple(c) for row in counts for c in row)


def _table(pairs):
    """pairs: ((rows, nodes), (table row, table node) where the segment starts)
    of every other rank in rank order -> the printed form of a segment table."""
    segs = [(p, at) for p, at in pairs if p[0] or p[1]]
    out = [len(segs)]
    rows = nodes = words = 0
    for (r, n), _ in segs + [((0, 0), None)]:
        out += [rows, nodes, words]
        rows, nodes, words = rows + r, nodes + n, words + r * ROW + n
    for _, at in segs:
        out += list(at)
    return out, rows, nodes, words


def restate(counts, world, rank):
    """What `xplan WORLD RANK counts` prints, as a list of integers, and the
    send / receive words."""
    mine = [tuple(c) for c in counts[rank]]
    e_lo, n_lo = sum(c[0] for c in mine[:rank]), sum(c[1] for c in mine[:rank])
    send, _, _, send_words = _table([(mine[d], (sum(c[0] for c in mine[:d]), sum(c[1] for c in mine[:d])))
                                     for d in range(world) if d != rank])
    recv, m, nm, recv_words = _table([(tuple(counts[q][rank]), (0, 0)) for q in range(world) if q != rank])
    any_ = any(tuple(counts[s][d]) != (0, 0) for s in range(world) for d in range(world) if s != d)
    too_large = m >= LIMIT or mine[rank][0] + m >= LIMIT or nm >= LIMIT
    head = [e_lo, mine[rank][0], n_lo, mine[rank][1], sum(c[0] for c in mine), sum(c[1] for c in mine),
            int(any_), int(too_large)]
    return head + send + recv, send_words, recv_words


def prefixes(line):
    """The (row, node, word) prefix tables of the send and the receive side of
    one printed plan."""
    v = [int(x) for x in line.split()]
    out, at = [], 8
    for _ in range(2):
        n = v[at]
        tri = v[at + 1:at + 1 + 3 * (n + 1)]
        out += [(n, tri[k::3]) for k in range(3)]
        at += 1 + 3 * (n + 1) + 2 * n
    assert at == len(v)
    return out


def _square(world, f):
    return [[f(s, d) for d in range(world)] for s in range(world)]


def _pattern(world, to_others, own=(6, 3)):
    """Every rank sends to_others[k] to the k-th other rank (in rank order)."""
    def f(s, d):
        return own if s == d else to_others[d - (d > s)]
    return _square(world, f)


def _two(own_rows, m, nm):
    """World 2, rank 0 keeps own_rows rows and receives m rows and nm nodes."""
    return [[(own_rows, 1), (0, 0)], [(m, nm), (2, 2)]]


MATRICES = {
    'world1': (1, [[(5, 9)]]),
    'world3': (3, _square(3, lambda s, d: (10 * s + d + 1, 100 * s + 7 * d))),
    'world32_full': (32, _square(32, lambda s, d: (s * 32 + d + 1, (s + 2 * d) % 5 + 1))),
    'diagonal': (4, _square(4, lambda s, d: (4 + s, 4) if s == d else (0, 0))),
    'only_to_last': (5, _square(5, lambda s, d: (3, 2) if s == d else (7, 1) if (s, d) == (1, 4) else (0, 0))),
    'nodes_only_between': (4, _pattern(4, [(3, 2), (0, 4), (5, 1)])),
    'empty_between': (4, _pattern(4, [(3, 2), (0, 0), (5, 1)])),
    'empty_own': (3, _pattern(3, [(2, 2), (4, 1)], own=(0, 0))),
    'rows_at_bound': (2, _two(0, LIMIT, 1)),
    'rows_below_bound': (2, _two(0, LIMIT - 1, 1)),
    'slots_at_bound': (2, _two(1, LIMIT - 1, 1)),
    'slots_below_bound': (2, _two(1, LIMIT - 2, 1)),
    'nodes_at_bound': (2, _two(0, 1, LIMIT)),
    'nodes_below_bound': (2, _two(0, 1, LIMIT - 1)),
}
