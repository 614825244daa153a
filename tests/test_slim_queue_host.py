"""The four-slot kernel's period queue, restated ("The period queue's tickets"; switch `claim_ahead`).

Two words in device memory: queue[0] hands out tickets, queue[1] counts the workgroups that have left.  A ticket below
n_periods is a period to search; a workgroup leaves on its first ticket at or above n_periods, and the last one to leave
rewinds both words for the next launch.  With the switch's bit 0 a workgroup's first ticket is its own index and the word
hands out blocks, blocks + 1, ...; without it every ticket comes from the word (the protocol the classic and the slab
kernels keep on the same words).  A period that re-enters the loop (`retry_exact`) keeps its ticket.

The model below is the kernel's protocol statement by statement, one scheduling step per statement that touches a queue
word; a seeded scheduler picks which workgroup moves next.  No GPU."""
import random

import pytest

BLOCKS = (1, 4, 1024)


def _counts(blocks):
    return sorted({0, 1, max(blocks - 1, 0), blocks, blocks + 1, 2 * blocks + 3})


class Queue(object):
    def __init__(self):
        self.words = [0, 0]
        self.draws = 0            # atomics on words[0]


class Workgroup(object):
    """tls_slim_kernel's period loop as far as the queue sees it."""

    def __init__(self, index, blocks, n_periods, bits, queue, searched, retries):
        self.index, self.blocks, self.n_periods, self.bits, self.queue = index, blocks, n_periods, bits, queue
        self.searched, self.retries = searched, retries
        self.work = -1                 # `int work = -1`: no ticket yet
        self.left = 0
        self.passes_left = 0
        self.state = "top"

    def ticket(self, first):           # slim_ticket
        if self.bits & 1 and first:
            return self.index
        self.queue.draws += 1
        got, self.queue.words[0] = self.queue.words[0], self.queue.words[0] + 1
        return (self.blocks if self.bits & 1 else 0) + got

    def step(self):
        assert self.state != "gone"
        if self.state == "top":                        # `if (!retry_exact)`: a fresh period
            self.work = self.ticket(self.work < 0)
            if self.work >= self.n_periods:
                self.state = "leave"
            else:
                self.passes_left = 1 + self.retries(self.work)   # the attempt, then the period's passes with `retry_exact`
                self.state = "search"
        elif self.state == "search":
            self.passes_left -= 1
            if self.passes_left == 0:
                self.searched.append(self.work)        # the period's result is written behind its last pass
                self.state = "top"
        elif self.state == "leave":
            self.left += 1
            done, self.queue.words[1] = self.queue.words[1], self.queue.words[1] + 1
            if done == self.blocks - 1:
                self.queue.words[0] = 0
                self.queue.words[1] = 0
            self.state = "gone"


def _launch(queue, blocks, n_periods, bits, pick, retries):
    searched = []
    wgs = [Workgroup(i, blocks, n_periods, bits, queue, searched, retries) for i in range(blocks)]
    live = list(range(blocks))
    steps = 0
    while live:
        at = pick(live)
        wg = wgs[live[at]]
        wg.step()
        if wg.state == "gone":
            live[at] = live[-1]
            live.pop()
        steps += 1
        assert steps <= 8 * (n_periods + blocks) + 16, "the launch does not end"
    return wgs, searched


def _schedulers(seed):
    rng = random.Random(seed)
    yield "random", lambda live: rng.randrange(len(live))
    yield "first to completion", lambda live: 0
    yield "last to completion", lambda live: len(live) - 1
    # bursts: one workgroup runs a few statements while the others stand still
    state = {"at": 0, "left": 0}

    def bursts(live):
        if state["left"] == 0 or state["at"] >= len(live):
            state["at"], state["left"] = rng.randrange(len(live)), rng.randrange(1, 7)
        state["left"] -= 1
        return state["at"]
    yield "bursts", bursts


@pytest.mark.parametrize("bits", [0, 1])
@pytest.mark.parametrize("blocks", BLOCKS)
def test_every_period_once_every_workgroup_leaves_once_and_the_words_rewind(blocks, bits):
    for n_periods in _counts(blocks):
        for seed in range(3 if blocks > 4 else 12):
            retry_rng = random.Random(1000 + seed)
            retry_of = {}

            def retries(work):     # a third of the periods go through the loop again once or twice on the same ticket
                if work not in retry_of:
                    retry_of[work] = retry_rng.choice((0, 0, 0, 0, 1, 2))
                return retry_of[work]
            for name, pick in _schedulers(seed):
                queue = Queue()
                for launch in range(2):                          # the second launch starts on the words the first left
                    what = (blocks, n_periods, bits, seed, name, launch)
                    wgs, searched = _launch(queue, blocks, n_periods, bits, pick, retries)
                    assert sorted(searched) == list(range(n_periods)), what
                    assert all(wg.left == 1 for wg in wgs), what
                    assert queue.words == [0, 0], what
                    # one atomic per ticket that is not a workgroup's own index
                    assert queue.draws == (launch + 1) * (n_periods + blocks - (blocks if bits & 1 else 0)), what


def test_a_workgroup_beyond_the_periods_never_touches_the_ticket_word():
    """Bit 0: its index is its one ticket at or above n_periods."""
    queue = Queue()
    wgs, searched = _launch(queue, 4, 1, 1, lambda live: len(live) - 1, lambda work: 0)
    assert searched == [0] and queue.words == [0, 0]
    assert queue.draws == 1          # workgroup 0, for the ticket it leaves on


def test_both_protocols_alternate_on_the_same_words():
    """The classic and the slab kernels count from zero on the same words: any order of families leaves them rewound."""
    queue = Queue()
    for launch, bits in enumerate((1, 0, 1, 1, 0, 0, 1)):
        rng = random.Random(launch)
        wgs, searched = _launch(queue, 4, 11, bits, lambda live: rng.randrange(len(live)), lambda work: work % 2)
        assert sorted(searched) == list(range(11)) and queue.words == [0, 0]
