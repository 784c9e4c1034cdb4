"""The two plain-Python helpers of the backward pass (dlwp_amd/backward.py) that need no device: GradBook's channel-window
arithmetic and SideLanes' fork / join sequences.  The expected sequences are derived by hand from Trainer._backward as it stood
before the pass moved into its own module; the lines they come from are quoted."""
import contextlib

from dlwp_amd.backward import GradBook, SideLanes


def _book(windows):
    book = GradBook(None, None, None, None)
    book.written[7] = list(windows)
    return book


def test_gradbook_windows():
    """overlaps:  any(not (c_off + c <= o or o + k <= c_off) for o, k in written.get(buf, []))
    covered:      all(any(o <= ch < o + k for o, k in written[buf]) for ch in range(c_off, c_off + c))"""
    book = _book([(0, 4), (8, 4)])
    # disjoint
    assert not book.overlaps(7, 4, 4) and not book.covered(7, 4, 4)
    assert not book.overlaps(7, 12, 3) and not book.covered(7, 12, 3)
    # nested: inside one window, and a window inside the query
    assert book.overlaps(7, 1, 2) and book.covered(7, 1, 2)
    assert book.overlaps(7, 0, 4) and book.covered(7, 0, 4)
    assert book.overlaps(7, 6, 8) and not book.covered(7, 6, 8)
    # partially overlapping: the case deposit refuses
    assert book.overlaps(7, 2, 4) and not book.covered(7, 2, 4)
    assert book.overlaps(7, 6, 3) and not book.covered(7, 6, 3)
    # touching at an edge: [4, 8) touches both windows, [3, 5) shares one channel with the first
    assert not book.overlaps(7, 4, 4)
    assert book.overlaps(7, 3, 2) and not book.covered(7, 3, 2)
    # two windows that touch cover a range across their common edge
    joined = _book([(0, 4), (4, 4)])
    assert joined.covered(7, 2, 4) and joined.overlaps(7, 2, 4) and not joined.covered(7, 2, 7)
    # a buffer nothing was written to
    assert not book.overlaps(3, 0, 4) and not book.covered(3, 0, 4)


class _Lanes(object):
    """SideLanes over named fake streams: log holds ('wait', waiter, waited-for) and ('run', function, current stream)."""

    def __init__(self, n_sides, n_wgrad, policy, capturing=False):
        self.log, self.current = [], 'main'
        sides = ['s%d' % i for i in range(n_sides)] if n_sides else None
        self.lanes = SideLanes(sides, 'main', n_wgrad, policy, capturing=capturing,
                               wait=lambda a, b: self.log.append(('wait', a, b)), on_stream=self.on_stream)

    @contextlib.contextmanager
    def on_stream(self, st):
        before, self.current = self.current, st
        try:
            yield
        finally:
            self.current = before

    def run(self, *names):
        for name in names:
            self.lanes.run(lambda name=name: self.log.append(('run', name, self.current)))


def test_side_lanes_each_policy_round_robins_and_waits_once_per_call():
    """    if each:
            st = sides[queued[0] % len(sides)]
            queued[0] += 1
            ops.stream_wait(st, main)
            if st not in used:
                used.append(st)
            with torch.cuda.stream(st):
                fn()
    ... and at the end:  for st in used: ops.stream_wait(main, st)"""
    t = _Lanes(2, 5, 'each')
    t.run('a', 'b', 'c')
    assert t.log == [('wait', 's0', 'main'), ('run', 'a', 's0'), ('wait', 's1', 'main'), ('run', 'b', 's1'),
                     ('wait', 's0', 'main'), ('run', 'c', 's0')]
    del t.log[:]
    t.lanes.join()
    assert t.log == [('wait', 'main', 's0'), ('wait', 'main', 's1')]
    # join waits on exactly the streams used: one function, three side streams
    t = _Lanes(3, 5, 'each')
    t.run('a')
    t.lanes.join()
    assert t.log == [('wait', 's0', 'main'), ('run', 'a', 's0'), ('wait', 'main', 's0')]


def test_side_lanes_batch_policy_flushes_at_the_half_and_at_the_end():
    """    wq.append(fn)
        queued[0] += 1
        if queued[0] == (n_wgrad + 1) // 2:
            launch_queued(False)
    launch_queued(parallel):  st = sides[i % len(sides)] if parallel else sides[0]; one stream_wait(st, main) per stream
    and call; at the end launch_queued(True), then for st in used: ops.stream_wait(main, st)"""
    t = _Lanes(2, 5, 'batch')
    t.run('a', 'b')
    assert t.log == []                                   # (5 + 1) // 2 = 3: nothing leaves before the third
    t.run('c')
    assert t.log == [('wait', 's0', 'main'), ('run', 'a', 's0'), ('run', 'b', 's0'), ('run', 'c', 's0')]
    del t.log[:]
    t.run('d', 'e', 'f')
    assert t.log == []
    t.lanes.join()
    assert t.log == [('wait', 's0', 'main'), ('run', 'd', 's0'), ('wait', 's1', 'main'), ('run', 'e', 's1'), ('run', 'f', 's0'),
                     ('wait', 'main', 's0'), ('wait', 'main', 's1')]
    # the first half alone used one stream: the join waits for that one only
    t = _Lanes(2, 2, 'batch')
    t.run('a')
    t.lanes.join()
    assert t.log == [('wait', 's0', 'main'), ('run', 'a', 's0'), ('wait', 'main', 's0')]


def test_side_lanes_without_side_streams_run_inline_and_in_order():
    """    if sides is None:
            return fn()
    ... if sides is not None: launch_queued(True); for st in used: ...   (nothing at the end)
    and, while capturing:  sides = None"""
    for t in (_Lanes(0, 4, 'each'), _Lanes(0, 4, 'batch'), _Lanes(2, 4, 'each', capturing=True),
              _Lanes(2, 4, 'batch', capturing=True)):
        t.run('a', 'b', 'c')
        t.lanes.join()
        assert t.log == [('run', 'a', 'main'), ('run', 'b', 'main'), ('run', 'c', 'main')]
