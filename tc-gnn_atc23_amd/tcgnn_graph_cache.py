"""What TCGNN.py keeps per graph, and when it lets go of it.  Pure bookkeeping: no library, no device - the owner hands in
destroy(handle), record_event(device, stream) -> event, event_done(event) -> bool and event_wait(event), so a test drives it
with integers for handles and flags for events (tests/test_graph_cache_cpu.py).

A CsrEntry, keyed by (nodePointer, edgeList), owns what is a function of those two tensors: the degree scales per norm and the
transposed CSR.  A PlanEntry, keyed by the five metadata tensors, owns the plan handle, the tensors kept alive, a reference to
its CsrEntry and - once a transpose=True call has asked for it - what such calls run on.  Whatever hangs off an entry leaves
with it.  Plan entries are bounded by `size`, least recently used first; so are, by the same code, the CSR entries no live plan
entry refers to (graphs only ever seen by degree_scales / transpose_graph).  An evicted plan is destroyed once an event recorded
at eviction time on every stream registered for its device has completed: nothing is synchronised."""
import collections

TransposedCsr = collections.namedtuple("TransposedCsr", "nodePointer_t edgeList_t perm symmetric")
TransposedPlan = collections.namedtuple("TransposedPlan", "plan own meta")   # own: the handle when it is A^T's own, else None (symmetric: A's plan, A's meta)


def graph_key(tensors):
    """A tensor is the one seen before while its storage address, length and in-place version counter are unchanged (entries
    keep their tensors alive, so an address can not be recycled under a live one)."""
    return tuple((t.data_ptr(), t.numel(), t._version) for t in tensors) + (tensors[0].device.index,)


class CsrEntry:
    __slots__ = ("key", "tensors", "scales", "transposed", "plans")

    def __init__(self, key, tensors):
        self.key, self.tensors = key, tensors
        self.scales = {}         # norm -> (row_scale, col_scale)
        self.transposed = None   # TransposedCsr, at first use
        self.plans = 0           # live plan entries that refer to this one


class PlanEntry:
    __slots__ = ("key", "handle", "tensors", "device", "csr", "transposed")

    def __init__(self, key, handle, tensors, device, csr):
        self.key, self.handle, self.tensors, self.device, self.csr = key, handle, tensors, device, csr
        self.transposed = None   # TransposedPlan, at first use

    def handles(self):
        own = self.transposed.own if self.transposed is not None else None
        return [self.handle] if own is None else [self.handle, own]


class GraphCache:
    def __init__(self, size, destroy, record_event, event_done, event_wait):
        self.size = max(1, int(size))
        self._destroy, self._record, self._done, self._wait = destroy, record_event, event_done, event_wait
        self._plans = collections.OrderedDict()      # plan key -> PlanEntry, least recently used first
        self._csrs = {}                              # CSR key -> CsrEntry, every live one
        self._planless = collections.OrderedDict()   # ... those of them with plans == 0, least recently used first
        self._retired = []                           # (events, evicted PlanEntry): kernels queued before the events may still read it
        self._streams = {}                           # device -> the streams plan-using calls were handed

    def register_stream(self, device, stream):
        self._streams.setdefault(device, set()).add(stream)

    def plan(self, key):
        e = self._plans.get(key)
        if e is not None:
            self._plans.move_to_end(key)
        return e

    def add_plan(self, key, handle, tensors, device):
        e = self._plans[key] = PlanEntry(key, handle, tensors, device, self.csr(tensors[:2], for_plan=True))
        self.trim()
        return e

    def csr(self, tensors, for_plan=False):
        """The entry of (nodePointer, edgeList), made at first sight.  for_plan: a new plan entry will refer to it."""
        key = graph_key(tensors)
        c = self._csrs.get(key)
        if c is None:
            c = self._csrs[key] = CsrEntry(key, tuple(tensors))
        if for_plan:
            self._planless.pop(key, None)
            c.plans += 1
        elif not c.plans:
            self._planless[key] = c
            self._planless.move_to_end(key)
            self._trim(self._planless, self._forget)
        return c

    def trim(self):
        """Bring both lists within `size` (the owner may have changed it), and destroy what has finished meanwhile"""
        self._trim(self._plans, self._retire)
        self._trim(self._planless, self._forget)
        self.reap()

    def _trim(self, lru, leave):
        while len(lru) > self.size:
            leave(lru.popitem(last=False)[1])

    def _forget(self, c):
        del self._csrs[c.key]

    def _retire(self, e, record=True):
        e.csr.plans -= 1
        if not e.csr.plans:
            self._forget(e.csr)
        events = [self._record(e.device, s) for s in self._streams.get(e.device, ())] if record else []
        self._retired.append((events, e))

    def reap(self, block=False):
        """Destroy the handles of retired entries whose every event has completed (block: wait for them)."""
        keep = []
        for events, e in self._retired:
            if block:
                for ev in events:
                    self._wait(ev)
            if all(self._done(ev) for ev in events):
                for h in e.handles():
                    self._destroy(h)
            else:
                keep.append((events, e))
        self._retired = keep

    def devices(self):
        return {e.device for e in self._plans.values()}

    def clear(self):
        """Everything goes, now.  The caller has synchronised devices(): live entries need no event."""
        while self._plans:
            self._retire(self._plans.popitem()[1], record=False)
        self.reap(block=True)
        self._csrs.clear()
        self._planless.clear()
        self._streams.clear()

    def stats(self):
        return dict(plans=len(self._plans), csrs=len(self._csrs), transposed=sum(e.transposed is not None for e in self._plans.values()),
                    retired=sum(len(e.handles()) for _, e in self._retired))
