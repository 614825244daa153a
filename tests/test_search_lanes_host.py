"""The launch lanes' choice of lane and their wait rules, restated ("Launch lanes"; tls_amd.hip:
main_stream, enqueue, update_flux_impl, tls_execute).

The model below is the host code statement by statement as far as streams, events and buffers go.  Every command it
enqueues becomes a node of a graph: a node is ordered behind the node before it on its stream and behind the record of
every event its stream has waited for.  Over random sequences of {execute, update_flux, fetch, prepare, counting execute}
the graph must order every two commands that touch the same buffer, one of them writing it -- two launches that share a
buffer set among them --, must order every consumer behind the latest launch and hand it that launch's results, and every
wait must name an event recorded EARLIER in host order (so the dependencies form a DAG).  No GPU."""
import random

import pytest


class Graph(object):
    def __init__(self):
        self.nodes = []          # (stream, reads, writes, what)
        self.before = []         # bit mask of the nodes a node is ordered behind
        self.last = {}           # stream -> its last node
        self.pending = {}        # stream -> nodes its next command is ordered behind through event waits
        self.events = {}         # event -> the node its latest record stands behind (None: an empty stream)
        self.waits = 0

    def record(self, event, stream):
        self.events[event] = self.last.get(stream)

    def wait(self, stream, event):
        assert event in self.events, "wait for %s, which no earlier command recorded" % event
        self.waits += 1
        if self.events[event] is not None:
            self.pending.setdefault(stream, []).append(self.events[event])

    def add(self, stream, reads, writes, what):
        behind = list(self.pending.pop(stream, []))
        if stream in self.last:
            behind.append(self.last[stream])
        mask = 0
        for p in behind:
            mask |= self.before[p] | (1 << p)
        me = len(self.nodes)
        for other, (_, r, w, other_what) in enumerate(self.nodes):
            if (w & (reads | writes)) or (r & writes):
                assert mask >> other & 1, "%s (node %d) is not ordered behind %s (node %d): they share %s" % (
                    what, me, other_what, other, sorted((w & (reads | writes)) | (r & writes)))
        self.nodes.append((stream, frozenset(reads), frozenset(writes), what))
        self.before.append(mask)
        self.last[stream] = me
        return me

    def ordered(self, first, then):
        return bool(self.before[then] >> first & 1)


class Context(object):
    """tls_ctx as far as the lanes go.  Buffers: plan, table, flux_a / flux_b, state_a / state_b (queue words, live-unit
    lists, stashed orders), out_a / out_b."""

    def __init__(self, lanes=True):
        self.g = Graph()
        self.lanes = lanes
        self.b_ready = False
        self.outstanding = False
        self.saw_state = False
        self.state_dirty = True
        self.run_lane = -1
        self.result_lane = 0
        self.flux_lane = 0
        self.flux_b_unseen = False
        self.a_reads_flux_b = self.b_reads_flux_a = False
        self.perm_filled = self.perm_filled_before_prev = False
        self.executed = False     # tls_fetch before tls_execute is an error: a new flux or plan has no results yet
        self.latest_launch = None
        self.launches = [0, 0]

    # -- lanes_join, main_stream
    def join(self):
        if self.outstanding:
            self.g.wait("A", "ev_done")
            self.outstanding = False
        self.flux_b_unseen = False
        self.b_reads_flux_a = False

    def main_stream(self):
        self.join()
        self.run_lane = -1
        self.state_dirty = True
        return "A"

    # -- ensure_lane_b, lane_b_see_state
    def ensure_lane_b(self):
        if not self.b_ready:
            self.g.add("B", set(), {"state_b"}, "lane B's queue words zeroed")
            self.b_ready = True

    def see_state(self):
        if not self.saw_state:
            self.g.wait("B", "ev_state")
            self.saw_state = True

    def overlappable(self):
        return self.lanes and self.perm_filled

    # -- tls_prepare (a new plan), update_flux_impl
    def prepare(self):
        stream = self.main_stream()
        self.perm_filled = self.perm_filled_before_prev = False
        self.result_lane = 0
        self.g.add(stream, set(), {"plan", "table", "flux_a"}, "plan upload")
        self.flux_lane = 0
        self.a_reads_flux_b = False
        self.executed = False

    def update_flux(self):
        self.executed = False
        if self.run_lane >= 0 and self.overlappable():
            target = self.run_lane ^ 1
            if (not self.a_reads_flux_b) if target == 1 else (not self.b_reads_flux_a):
                if target == 1:
                    self.ensure_lane_b()
                    self.see_state()
                    self.g.add("B", set(), {"flux_b"}, "flux upload on lane B")
                    self.g.record("ev_stage_b", "B")
                    self.g.record("ev_done", "B")
                    self.outstanding = True
                    self.flux_b_unseen = True
                    self.flux_lane = 1
                else:
                    self.g.add("A", set(), {"flux_a"}, "flux upload on lane A")
                    self.state_dirty = True
                    self.flux_lane = 0
                return
        self.flux_lane = 0
        self.g.add(self.main_stream(), set(), {"flux_a"}, "flux upload, joined")

    # -- tls_execute, enqueue
    def execute(self, counting=False):
        lane = -1
        if not counting and self.perm_filled_before_prev and self.overlappable():
            lane = 1 if self.run_lane == 0 else 0
        filled_before = self.perm_filled
        if lane < 0:
            stream = self.main_stream()
        elif lane == 0:
            stream = "A"
            if self.state_dirty:
                self.g.record("ev_state", stream)
                self.state_dirty = False
                self.saw_state = False
                self.a_reads_flux_b = False
            if self.flux_lane == 1 and self.flux_b_unseen:
                self.g.wait(stream, "ev_stage_b")
                self.flux_b_unseen = False
        else:
            self.ensure_lane_b()
            self.see_state()
            stream = "B"
        if self.flux_lane == 1 and lane != 1:
            self.a_reads_flux_b = True
        if self.flux_lane == 0 and lane == 1:
            self.b_reads_flux_a = True
        side = "b" if lane == 1 else "a"
        self.result_lane = 1 if lane == 1 else 0
        reads = {"plan", "flux_b" if self.flux_lane == 1 else "flux_a"}
        writes = {"out_" + side, "state_" + side}
        if self.perm_filled:
            reads.add("table")
        else:
            writes.add("table")
            assert lane < 0, "the filling launch overlaps nothing"
        self.latest_launch = self.g.add(stream, reads, writes, "launch on lane %s%s" % (side.upper(), "" if lane >= 0 else " (joined)"))
        self.perm_filled = True
        self.executed = True
        if lane == 1:
            self.g.record("ev_done", stream)
            self.outstanding = True
        self.perm_filled_before_prev = filled_before
        self.run_lane = lane
        self.launches[1 if lane == 1 else 0] += 1
        return lane

    # -- tls_fetch and every other consumer of the results
    def fetch(self):
        node = self.g.add(self.main_stream(), {"out_b" if self.result_lane == 1 else "out_a"}, set(), "fetch")
        assert self.executed and self.g.ordered(self.latest_launch, node), "the fetch is not behind the latest launch"
        _, _, writes, _ = self.g.nodes[self.latest_launch]
        assert ("out_b" if self.result_lane == 1 else "out_a") in writes, "the fetch reads another lane's results"


OPS = ("execute", "update_flux", "fetch", "prepare", "counting")


@pytest.mark.parametrize("seed", range(40))
@pytest.mark.parametrize("lanes", [True, False], ids=["lanes_on", "lanes_off"])
def test_random_sequences_are_ordered(seed, lanes):
    rng = random.Random(seed)
    ctx = Context(lanes)
    ctx.prepare()
    ctx.execute()
    weights = [rng.choice((8, 20)), rng.choice((1, 6, 12)), rng.choice((1, 3)), rng.choice((0, 1)), rng.choice((0, 1))]
    for _ in range(120):
        op = rng.choices(OPS, weights)[0]
        if op == "execute":
            ctx.execute()
        elif op == "counting":
            ctx.execute(counting=True)
        elif op == "update_flux":
            ctx.update_flux()
        elif op == "prepare":
            ctx.prepare()
        elif ctx.executed:
            ctx.fetch()
    if ctx.executed:
        ctx.fetch()
    assert lanes or ctx.launches[1] == 0


def test_an_unbroken_run_alternates_and_waits_for_nothing():
    """fill, read, then A, B, A, B, ...: one record of lane A's state, one wait for it on lane B, and no other wait -- the
    steady state of back-to-back searches costs no event at all."""
    ctx = Context()
    ctx.prepare()
    assert [ctx.execute() for _ in range(8)] == [-1, -1, 0, 1, 0, 1, 0, 1]
    assert ctx.g.waits == 1
    ctx.fetch()
    assert ctx.g.waits == 2      # the join
    assert [ctx.execute() for _ in range(3)] == [0, 1, 0]


def test_streaming_keeps_a_flux_per_lane():
    """update_flux and execute alternating: the flux goes to the lane the next search takes, and no launch reads the other
    lane's flux -- so no upload ever joins."""
    ctx = Context()
    ctx.prepare()
    for _ in range(3):
        ctx.update_flux()
        ctx.execute()
    lanes = []
    for _ in range(8):
        ctx.update_flux()
        assert not ctx.a_reads_flux_b and not ctx.b_reads_flux_a
        lanes.append(ctx.execute())
    assert lanes == [1, 0, 1, 0, 1, 0, 1, 0]
    assert all("joined" not in what for _, _, _, what in ctx.g.nodes[-16:])


def test_a_consumer_between_two_searches_leaves_the_next_on_lane_a():
    ctx = Context()
    ctx.prepare()
    for _ in range(3):
        ctx.execute()
    for _ in range(5):
        ctx.fetch()
        assert ctx.execute() == 0
    assert ctx.execute() == 1
    assert ctx.execute(counting=True) == -1
    assert ctx.execute() == 0
