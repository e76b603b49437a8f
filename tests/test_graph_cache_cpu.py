"""tcgnn_graph_cache.GraphCache - the bookkeeping behind TCGNN.py's plans, transposed parts, degree scales and transposed CSRs - driven
without a library or a device: handles are integers, events are flags the test flips, tensors are CPU tensors (graph_key reads their
address, length and version counter only)."""
import collections
import random

import pytest
import torch

from tcgnn_graph_cache import GraphCache, TransposedCsr, TransposedPlan, graph_key


class Event:
    def __init__(self, device, stream):
        self.device, self.stream, self.complete = device, stream, False


class World:
    """The callables the cache is handed, recording what it does with them, and a model of the plan LRU of the test's own: it says
    which entries each look-up evicts, so every retired handle is tied to the events recorded at its eviction."""

    def __init__(self, size):
        self.events, self.destroyed, self.pending, self.next_handle = [], [], {}, 0
        self.size, self.model = size, collections.OrderedDict()   # plan key -> its handles, least recently used first
        self.cache = GraphCache(size, self.destroy, self.record, lambda e: e.complete, self.wait)

    def record(self, device, stream):
        self.events.append(Event(device, stream))
        return self.events[-1]

    def wait(self, event):
        event.complete = True

    def destroy(self, handle):
        assert handle in self.pending, "handle %d destroyed while its entry is live" % handle
        assert all(e.complete for e in self.pending[handle]), "handle %d destroyed under an incomplete event" % handle
        self.destroyed.append(handle)

    def handle(self):
        self.next_handle += 1
        return self.next_handle

    def look_up(self, meta, device=0, transpose=False):
        """What a plan look-up of TCGNN.py does (transpose: with the part such calls run on), a counter in place of tcgnn_plan_create"""
        key = graph_key(meta)
        before = len(self.events)
        e = self.cache.plan(key)
        assert (e is None) == (key not in self.model)
        if e is None:
            self.model[key] = [self.next_handle + 1]
            while len(self.model) > self.size:
                for h in self.model.popitem(last=False)[1]:
                    self.pending[h] = self.events   # (the slice is taken below, once the cache has recorded)
            e = self.cache.add_plan(key, self.handle(), meta, device)
            for h, ev in self.pending.items():
                if ev is self.events:
                    self.pending[h] = self.events[before:]
        else:
            self.model.move_to_end(key)
        if transpose and e.transposed is None:
            if e.csr.transposed is None:
                e.csr.transposed = TransposedCsr("rp_t", "col_t", "perm", False)
            own = self.handle()
            e.transposed = TransposedPlan(own, own, ("meta_t",))
            self.model[key].append(own)
        assert self.cache.stats()["plans"] == len(self.model)
        return e

    def clear(self):
        for handles in self.model.values():
            for h in handles:
                self.pending[h] = []
        self.model.clear()
        self.cache.clear()


def graph(seed):
    """five CPU int32 tensors standing for nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow"""
    return tuple(torch.full((4 + i,), seed, dtype=torch.int32) for i in range(5))


@pytest.mark.parametrize("size", [1, 3, 8])
def test_every_handle_is_destroyed_once_and_never_under_an_incomplete_event(size):
    w = World(size)
    graphs = [graph(seed=k) for k in range(12)]
    rng = random.Random(size)
    w.cache.register_stream(0, 0)
    w.cache.register_stream(0, 77)
    for step in range(200):
        w.look_up(graphs[rng.randrange(12)], transpose=rng.random() < 0.4)
        if rng.random() < 0.3:                      # some of the queued work finishes
            for e in rng.sample(w.events, len(w.events) // 2):
                e.complete = True
        if step % 17 == 0:
            w.cache.csr(graphs[rng.randrange(12)][:2]).scales["both"] = ("r", "c")
        s = w.cache.stats()
        assert s["plans"] <= size and s["transposed"] <= s["plans"]
        assert s["csrs"] <= 2 * size                # (those with a plan, and as many without)
        assert len(w.destroyed) == len(set(w.destroyed))
    assert w.next_handle > size                     # (the script did evict)
    w.clear()
    assert sorted(w.destroyed) == list(range(1, w.next_handle + 1))
    assert w.cache.stats() == dict(plans=0, csrs=0, transposed=0, retired=0)


def test_a_retired_plan_waits_for_every_event_of_its_eviction():
    w = World(1)
    w.cache.register_stream(0, 0)
    w.cache.register_stream(0, 5)
    a, b, c = graph(seed=1), graph(seed=2), graph(seed=3)
    w.look_up(a, transpose=True)                    # handles 1 (A) and 2 (A^T's own)
    w.look_up(b)                                    # evicts a
    assert len(w.events) == 2 and w.destroyed == [] and w.cache.stats()["retired"] == 2
    w.events[0].complete = True
    w.cache.reap()
    assert w.destroyed == []
    w.events[1].complete = True
    w.look_up(c)                                    # a later miss reaps (and retires b)
    assert sorted(w.destroyed) == [1, 2] and w.cache.stats()["retired"] == 1
    w.cache.reap(block=True)
    assert sorted(w.destroyed) == [1, 2, 3]


def test_eviction_releases_the_transposed_part_and_a_csr_entry_nobody_else_uses():
    w = World(2)
    a = graph(seed=1)
    a2 = a[:2] + (torch.full((9,), 1, dtype=torch.int32),) + a[3:]      # same (nodePointer, edgeList), another blockPartition
    b, c = graph(seed=2), graph(seed=3)
    ea, ea2 = w.look_up(a, transpose=True), w.look_up(a2)
    assert ea is not ea2 and ea.csr is ea2.csr and ea.csr.plans == 2
    ea.csr.scales["both"] = ("r", "c")
    assert w.cache.stats() == dict(plans=2, csrs=1, transposed=1, retired=0)
    w.look_up(b)                                    # evicts a: its own A^T handle goes with it, the CSR entry stays for a2
    assert w.cache.stats() == dict(plans=2, csrs=2, transposed=0, retired=0)   # (no stream registered: nothing to wait for)
    assert sorted(w.destroyed) == [ea.handle, ea.transposed.own]
    assert w.cache.csr(a[:2]) is ea2.csr and ea2.csr.scales == {"both": ("r", "c")} and ea2.csr.transposed is not None
    w.look_up(c)                                    # evicts a2: the last reference to the CSR entry
    assert w.cache.stats() == dict(plans=2, csrs=2, transposed=0, retired=0)
    fresh = w.cache.csr(a[:2])
    assert fresh is not ea2.csr and fresh.scales == {} and fresh.transposed is None and fresh.plans == 0


def test_planless_csr_entries_count_against_the_limit_least_recently_used_first():
    w = World(2)
    g = [graph(seed=k)[:2] for k in range(4)]
    c0, c1 = w.cache.csr(g[0]), w.cache.csr(g[1])
    assert w.cache.csr(g[0]) is c0                  # a look-up: g[1] is now the least recently used
    c2 = w.cache.csr(g[2])
    assert w.cache.stats()["csrs"] == 2
    assert w.cache.csr(g[0]) is c0 and w.cache.csr(g[2]) is c2
    assert w.cache.csr(g[1]) is not c1              # (dropped; this makes it anew and drops g[0])
    assert w.cache.csr(g[0]) is not c0
    # an entry that gets a plan no longer counts against the planless limit (it will leave with its last plan)
    full = graph(seed=9)
    c9 = w.cache.csr(full[:2])
    assert w.look_up(full).csr is c9 and c9.plans == 1
    w.cache.csr(g[2]), w.cache.csr(g[3])
    assert w.cache.csr(full[:2]) is c9 and w.cache.stats()["csrs"] == 3
    w.cache.size = 1
    w.cache.trim()
    assert w.cache.stats() == dict(plans=1, csrs=2, transposed=0, retired=0)


@pytest.mark.parametrize("which", range(5))
def test_a_changed_version_counter_is_a_miss(which):
    w = World(4)
    meta = graph(seed=1)
    e = w.look_up(meta)
    assert w.look_up(meta) is e and w.next_handle == 1
    meta[which].add_(0)                             # in place: same storage, same length, the version counter moves
    e2 = w.look_up(meta)
    assert e2 is not e and w.next_handle == 2
    assert (e2.csr is e.csr) == (which >= 2)        # (nodePointer and edgeList are the CSR entry's key)


def test_events_are_asked_for_every_registered_stream_of_the_evicted_plans_device_only():
    w = World(1)
    w.cache.register_stream(0, 0)
    w.cache.register_stream(0, 11)
    w.cache.register_stream(0, 11)
    w.cache.register_stream(0, 12)                  # a prepare-style call: a stream no buffer was ever asked for on
    w.cache.register_stream(1, 21)
    on0, on1 = graph(seed=1), graph(seed=2)
    w.look_up(on0, device=0)
    w.look_up(on1, device=1)                        # evicts the plan of device 0
    assert sorted((e.device, e.stream) for e in w.events) == [(0, 0), (0, 11), (0, 12)]
    del w.events[:]
    w.look_up(on0, device=0)                        # evicts the plan of device 1
    assert [(e.device, e.stream) for e in w.events] == [(1, 21)]
