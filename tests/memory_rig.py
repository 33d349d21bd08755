"""The memory-contract rig: does a call stay inside the region it declared, and does it depend on what the region held?

include/conv3p.h promises about every caller-owned region (`workspace`, `scratch`, `cache`) that all scratch comes from it,
that its size comes from the matching `*_bytes` export, and, for the per-call ones, that it "need not be initialised and
nothing is kept in it between calls".  A C caller allocates exactly the declared size; the Python mirror's pooled
workspaces are far larger at test shapes and are reused, so an overrun or a read of a stale word goes unseen.  This rig
puts every region at exactly the size the call was given, between guards, and fills it:

  Arena      one tensor laid out guard | body | guard.  The body is exactly the declared byte count; base and body are
             256-byte aligned; each guard is as wide as the body, at least 64 KiB and at most 16 MiB (conditions, not
             measurements: an overrun of up to the region's own size lands in memory the test owns) and holds the
             position-dependent pattern (131 i + 7) & 0xFF, so that a memset-style overrun shows too.  intact() compares
             both guards with the pattern and reports the first and last changed offset relative to the body.
  Regions    the arenas of one case, by (function, region, n-th call of the run): enter() hands out the body, pre-filled
             with the chosen fill on the current stream.  Shim (below) is its ctypes-level form: while a case's run() is
             on the stack it swaps the pointer and byte count of every per-call region for such a body.
  judge()    the rules for one case: R1 bounds (every guard of every region the call touched is intact after every
             run), R2 dirty contents (runs on bodies filled with 0x00, with 0xFF and with the leftover of the poison
             half's run give bit-identical outputs), and the outputs themselves for R3.  short_run() is R0: the same
             call with one byte less is refused with CONV3P_ERR_WORKSPACE (REFUSES_WITH: the status the function's own
             paragraph documents) and leaves the outputs, the body of a region that keeps state and all guards alone.

Regions that keep state (KEEPS_STATE: the neighbour cache) are not substituted -- the library keys host bookkeeping by
their address -- but made arena bodies where their owner allocates them (cache_in_arena()); they get R0 and R1, not R2.

The plants at the bottom are plain torch on the rig's own arenas: they write inside the arena only, so the rig cannot
form a bad address.  The module is device-agnostic: tests/test_memory_contract_host.py runs its logic on CPU tensors.
"""
import collections
import gc
import os
import re
import warnings

import torch

from tests.stream_rig import _same

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "conv3p.h")
REGION_NAMES = ("workspace", "scratch", "cache")
ALIGN = 256
GUARD_MIN, GUARD_MAX = 64 << 10, 16 << 20
ERR_WORKSPACE = 2                                        # CONV3P_ERR_WORKSPACE
FILLS = collections.OrderedDict([("0x00", 0x00), ("0xFF", 0xFF)])     # + "leftover": what the poison half's run left
SENTINEL = 0xA5                                          # what R0 puts into the outputs of the call to be refused

# Regions the header says keep state between calls, with the sentence that says so.  Every function that takes a
# `cache` shares the first sentence (the section comment of the *_cached entry points, which the stack's comment refers
# to: "`cache` as for the *_cached entry points"); conv3p_cache_init is the call that establishes it.
_CACHE = "The *_cached entry points keep that state in a caller-owned, persistent device buffer:"
_CACHE_STACK = "`cache` as for the *_cached entry points, with slots >= number of distinct strides."
_CACHE_INIT = "Make `cache` (cache_bytes of freshly allocated, possibly RECYCLED device memory) a valid empty cache: zero-fills it on"
KEEPS_STATE = {"conv3p_cache_init": {"cache": _CACHE_INIT}}
for _sfx in ("f32", "f64"):
    for _fn in ("forward_cached", "backward_cached", "cache_prepare", "cache_prepare_multi", "layer_forward_cached",
                "layer_backward_cached"):
        KEEPS_STATE["conv3p_%s_%s" % (_fn, _sfx)] = {"cache": _CACHE}
    for _fn in ("stack_prefetch", "stack_forward", "stack_backward"):
        KEEPS_STATE["conv3p_%s_%s" % (_fn, _sfx)] = {"cache": _CACHE_STACK}
# (`scratch` of conv3p_stack_backward_* is a per-call region: the header calls it the "bytes of scratch
# conv3p_stack_backward_* needs", the forward does not take it, and nothing says it is kept.  It gets every rule.)

# Functions whose region has no declared size to be one byte short of, and why.
NO_DECLARED_SIZE = {
    "conv3p_cache_init": "cache_bytes is how much the call zero-fills, whatever the caller says: no *_bytes export bounds it",
}

# Functions whose own paragraph of the header states ANOTHER status for a short workspace than the general
# CONV3P_ERR_WORKSPACE ("workspace NULL, misaligned (256 B) or too small"), with that sentence (comment line breaks
# flattened): R0 expects the documented status there; everything else about a refused call is the same.
ERR_INVALID_ARGUMENT = 1
_SEGMENTS = ("workspace NULL or smaller than conv3p_grid_segments_workspace_bytes(M) / "
             "conv3p_grid_absorb_workspace_bytes(M): CONV3P_ERR_INVALID_ARGUMENT.")
_RINGS = ("workspace NULL or smaller than conv3p_grid_interpolate_rings_workspace_bytes(N) (a counter and an int32 per row): "
          "CONV3P_ERR_INVALID_ARGUMENT.")
REFUSES_WITH = {
    "conv3p_grid_interpolate_rings_f32": (ERR_INVALID_ARGUMENT, _RINGS),
    "conv3p_grid_interpolate_rings_i64": (ERR_INVALID_ARGUMENT, _RINGS),
    "conv3p_grid_segments": (ERR_INVALID_ARGUMENT, _SEGMENTS),
    "conv3p_grid_segments_smooth": (ERR_INVALID_ARGUMENT, "Status: those of conv3p_grid_segments in its order"),
    "conv3p_grid_absorb_segments": (ERR_INVALID_ARGUMENT, _SEGMENTS),
    "conv3p_grid_segment_adjacency": (ERR_INVALID_ARGUMENT, "workspace NULL or smaller than conv3p_grid_adjacency_scratch_bytes(M, "
                                      "max_edges): CONV3P_ERR_INVALID_ARGUMENT."),
    "conv3p_grid_merge_segments": (ERR_INVALID_ARGUMENT, "workspace NULL or smaller than conv3p_grid_merge_scratch_bytes(M): "
                                   "CONV3P_ERR_INVALID_ARGUMENT."),
}


def flat_header(header=HEADER):
    """The header's text with the line breaks inside comments (newline, ` * `, indentation) made single spaces."""
    return re.sub(r"\s*\n\s*\*?\s*", " ", open(header).read())


# ------------------------------------------------------------------------------------------------ the region finder
def _declarations(header=HEADER):
    text = re.sub(r"/\*.*?\*/", " ", open(header).read(), flags=re.S)
    return [(name, [p.strip() for p in params.split(",")])
            for name, params in re.findall(r"\b(conv3p_\w+)\s*\(([^;{}()]*)\)\s*;", text)]


def regions(header=HEADER):
    """{function: [(region, position of `void *X`, position of `size_t X_bytes`)]} for every function of the header
    with such a pair, X in REGION_NAMES; positions count the C parameters from 0.  A function declared twice raises."""
    found = {}
    for name, params in _declarations(header):
        pairs = []
        for i, p in enumerate(params[:-1]):
            m = re.fullmatch(r"void\s*\*\s*(\w+)", p)
            if m and m.group(1) in REGION_NAMES and re.fullmatch(r"size_t\s+%s_bytes" % m.group(1), params[i + 1]):
                pairs.append((m.group(1), i, i + 1))
        if pairs:
            assert name not in found, "%s is declared twice" % name
            found[name] = pairs
    return found


def output_positions(header=HEADER):
    """{function: positions of its parameters `T *name` with T neither const nor void}: the device tensors a call may
    write (tables of pointers, `T *const *`, are host arrays and are left out)."""
    out = {}
    for name, params in _declarations(header):
        out[name] = [i for i, p in enumerate(params)
                     if re.fullmatch(r"(?!const\b)(?!void\b)\w+\s*\*\s*\w+", p)]
    return out


# ------------------------------------------------------------------------------------------------ the arena
def guard_bytes(nbytes):
    g = min(max(int(nbytes), GUARD_MIN), GUARD_MAX)
    return (g + ALIGN - 1) // ALIGN * ALIGN


_PATTERN = {}


def _pattern(n, device):
    """(131 i + 7) & 0xFF for i in [0, n) on `device`, from one growing tensor per device."""
    key = str(torch.device(device))
    p = _PATTERN.get(key)
    if p is None or p.numel() < n:
        i = torch.arange(max(n, GUARD_MIN), dtype=torch.int32, device=device) & 0xFF   # (the same residue mod 256)
        p = _PATTERN[key] = ((i * 131 + 7) & 0xFF).to(torch.uint8)
    return p[:n]


class Arena:
    """guard | body | guard in one tensor; see the module docstring."""

    def __init__(self, nbytes, device, label=""):
        assert nbytes > 0
        self.nbytes, self.label = int(nbytes), label
        self.guard = g = guard_bytes(nbytes)
        self.raw = torch.empty(2 * g + self.nbytes + ALIGN, dtype=torch.uint8, device=device)
        off = -self.raw.data_ptr() % ALIGN
        self.low = self.raw[off:off + g]
        self.body = self.raw[off + g:off + g + self.nbytes]
        self.high = self.raw[off + g + self.nbytes:off + 2 * g + self.nbytes]
        self.base = self.low.data_ptr()
        self.low.copy_(_pattern(g, device))
        self.high.copy_(_pattern(g, device))

    def fill(self, value):
        """The body set to a byte value, on the current stream; None leaves what it holds."""
        if value is not None:
            self.body.fill_(value)

    def intact(self):
        """None if both guards hold the pattern, else (first, last) changed offset relative to the body: negative below
        it, >= nbytes above.  Reads the device: call after a synchronise."""
        first = last = None
        for guard, start in ((self.low, -self.guard), (self.high, self.nbytes)):
            bad = guard != _pattern(self.guard, guard.device)
            if bool(bad.any()):
                where = torch.nonzero(bad).flatten()
                lo, hi = start + int(where[0]), start + int(where[-1])
                first = lo if first is None else min(first, lo)
                last = hi if last is None else max(last, hi)
        return None if first is None else (first, last)

    def mend(self):
        """The guards put back, so that one violation is reported once."""
        self.low.copy_(_pattern(self.guard, self.low.device))
        self.high.copy_(_pattern(self.guard, self.high.device))


class Regions:
    """The arenas of one case.  enter(function, region, nbytes, device) -> the arena of the n-th such call of this run,
    its body pre-filled with self.fill (a byte value; None: left as it is) on the current stream."""

    def __init__(self):
        self.fill = None
        self.arenas = collections.OrderedDict()          # (function, region, n) -> Arena
        self.touched = []                                # keys entered during the current run, in order
        self._n = collections.Counter()

    def begin_run(self, fill):
        self.fill = fill
        self.touched = []
        self._n.clear()

    def enter(self, function, region, nbytes, device):
        n = self._n[function, region]
        self._n[function, region] += 1
        key = (function, region, n)
        a = self.arenas.get(key)
        if a is None or a.nbytes != nbytes:
            a = self.arenas[key] = Arena(nbytes, device, "%s: `%s` (call %d of the run)" % key)
        a.fill(self.fill)
        self.touched.append(key)
        return a

    def adopt(self, function, region, arena):
        """A region that keeps state, allocated as an arena by its owner: noted as touched, never filled."""
        key = (function, region, id(arena))
        self.arenas[key] = arena
        if key not in self.touched:
            self.touched.append(key)

    def changed(self):
        """{label: (first, last)} of the touched arenas whose guards changed; those guards are mended."""
        out = collections.OrderedDict()
        for key in self.touched:
            a = self.arenas[key]
            r = a.intact()
            if r is not None:
                out["%s: `%s`, %d bytes" % (key[0], key[1], a.nbytes)] = r
                a.mend()
        return out


def _sync(device):
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize(device)


def _host(outs):
    outs = list(outs) if isinstance(outs, (list, tuple)) else [outs]
    return [t.detach().cpu().clone() for t in outs]


def differing(a, b):
    """Indices of the outputs that differ bit for bit (-1: another number of outputs)."""
    return [i for i, (x, y) in enumerate(zip(a, b)) if not _same(x, y)] + ([-1] if len(a) != len(b) else [])


Verdict = collections.namedtuple("Verdict", "outputs changed dirty sizes")


def judge(case, regs, device, leftover=True):
    """R1 and R2 for one case.  case: a stream_rig.Case whose run() enters `regs`; returns
      outputs  {fill: host copies of run()'s outputs}, fills "0x00", "0xFF" and "leftover";
      changed  {fill: {region label: (first, last) changed guard offset}}, empty values where R1 holds;
      dirty    {fill: indices of the outputs that differ from the 0x00 run's}, empty values where R2 holds;
      sizes    {region label: bytes} of every region the runs entered."""
    outputs, changed = collections.OrderedDict(), collections.OrderedDict()
    real = [x.clone() for x in case.inputs]

    def one(name, fill):
        case.reset()
        regs.begin_run(fill)
        outs = case.run()
        _sync(device)
        outputs[name] = _host(outs)
        changed[name] = regs.changed()

    for name, fill in FILLS.items():
        one(name, fill)
    if leftover:
        for x, p in zip(case.inputs, case.poison):
            x.copy_(p)
        one("poison", 0x5A)                              # the other half's run: its leftovers stay in the bodies
        for x, r in zip(case.inputs, real):
            x.copy_(r)
        one("leftover", None)
        del outputs["poison"]
    first = next(iter(outputs))
    dirty = collections.OrderedDict((name, differing(outputs[first], outs)) for name, outs in outputs.items())
    sizes = collections.OrderedDict(("%s: `%s` #%s" % key, a.nbytes) for key, a in regs.arenas.items())
    return Verdict(outputs, changed, dirty, sizes)


def describe(changed):
    return "; ".join("[%s] %s guard bytes %d .. %d relative to the body changed" % (fill, label, r[0], r[1])
                     for fill, per in changed.items() for label, r in per.items())


# ------------------------------------------------------------------------------------------------ the ctypes shim
def exact_workspace(dev, nbytes, pool):
    """Stands in for pointwise_amd._host._workspace in the modules that import it by name: the pool's buffer cut to
    exactly `nbytes`, so that the `ws.numel()` the wrappers pass on is the declared need (the product's floor stays)."""
    from pointwise_amd import _host
    return _host._workspace(dev, nbytes, pool)[:nbytes]


WORKSPACE_IMPORTERS = ("conv3p_op", "head", "seg_head", "optim")      # `from ._host import _workspace`


def patch_workspace_floor(monkeypatch):
    import importlib
    for mod in WORKSPACE_IMPORTERS:
        monkeypatch.setattr(importlib.import_module("pointwise_amd." + mod), "_workspace", exact_workspace)


_CACHE_ARENAS = {}                                       # body address -> Arena, of the caches made under cache_in_arena()


def cache_in_arena(monkeypatch):
    """NeighborCache.__init__ wrapped: the cache's buffer becomes the zero-filled body of an arena of exactly
    conv3p_cache_bytes (its owner allocates it; the library keys its bookkeeping by that address)."""
    from pointwise_amd import conv3p_op

    init = conv3p_op.NeighborCache.__init__

    def wrapped(self, *args, **kw):
        init(self, *args, **kw)
        a = Arena(self.nbytes, self.buf.device, "NeighborCache.buf")
        a.body.zero_()
        self.buf = a.body
        self._arena = a                                  # lives as long as the cache
        _CACHE_ARENAS[a.body.data_ptr()] = a
    monkeypatch.setattr(conv3p_op.NeighborCache, "__init__", wrapped)


class TensorIndex:
    """Where R0 finds the tensors behind a call's output pointers without looking at every object of the process for every
    case: the device tensors alive now, then gc.freeze(), after which gc.get_objects() lists only what was made since
    (close() undoes it).  One per test module; the tensors found at the start are held."""

    def __init__(self, device):
        self.device, self.base = device, {}
        _note_tensors(self.base, gc.get_objects(), device)
        gc.freeze()

    def tensors(self):
        """{address: the largest live contiguous tensor on the device that starts there}."""
        found = dict(self.base)
        _note_tensors(found, gc.get_objects(), self.device)
        return found

    def close(self):
        gc.unfreeze()


class Shim(Regions):
    """Shims around the functions of the loaded library that take a region, active only while a case's run() is on the
    stack (around()).  A per-call region's pointer and byte count are swapped for an arena body of the size the call was
    given; a region that keeps state must already be the body of an arena of that size (cache_in_arena) and is noted.
    In a short run (R0) every such call is first made with one byte less, region by region, see short_run()."""

    def __init__(self, lib, device, index=None, header=HEADER):
        Regions.__init__(self)
        self.lib, self.device, self.index = lib, device, index
        self.table = regions(header)
        self.outputs = output_positions(header)
        self.active = self.short = False
        self.originals = {}
        self.refusals = []                               # R0: (function, region, what went wrong or "")
        self.not_arenas = []                             # state-keeping regions that were no arena of their size
        self._old_tensors = {}

    def __enter__(self):
        for name in self.table:
            fn = getattr(self.lib, name)
            self.originals[name] = fn
            setattr(self.lib, name, self._shim(name, fn))
        return self

    def __exit__(self, *exc):
        for name, fn in self.originals.items():
            setattr(self.lib, name, fn)

    def around(self, case):
        def run():
            self.active = True
            try:
                return case.run()
            finally:
                self.active = False
        return case._replace(run=run)

    def _shim(self, name, fn):
        def call(*args):
            if not self.active:
                return fn(*args)
            args = list(args)
            mine = []                                    # (region, position of the byte count, arena, keeps state)
            for region, p, b in self.table[name]:
                ptr, nbytes = args[p], args[b]
                ptr = getattr(ptr, "value", ptr)
                if not ptr or not nbytes:
                    continue                             # the call has no such region this time
                if region in KEEPS_STATE.get(name, {}):
                    a = _CACHE_ARENAS.get(ptr)
                    if a is None or a.nbytes != nbytes:
                        self.not_arenas.append((name, region, nbytes))
                        continue
                    self.adopt(name, region, a)
                    mine.append((region, b, a, True))
                else:
                    a = self.enter(name, region, int(nbytes), self.device)
                    args[p] = a.body.data_ptr()
                    mine.append((region, b, a, False))
            if self.short and name not in NO_DECLARED_SIZE:
                for region, b, a, _ in mine:
                    self._refused(name, fn, args, region, b, mine)
            return fn(*args)
        return call

    # ---- R0
    def _tensors(self):
        """{address: the largest live contiguous tensor on the device that starts there}."""
        found = dict(self._old_tensors)
        _note_tensors(found, gc.get_objects(0), self.device)
        return found

    def _refused(self, name, fn, args, region, b, mine):
        """The call with one byte less of `region`: refused, and its outputs, the body of every region that keeps state
        and all guards unchanged.  (The body of a per-call region is the call's to write whatever it returns: a call may
        have enqueued work on its own scratch before it finds another region short.)"""
        short = list(args)
        short[b] = args[b] - 1
        tensors = self._tensors()
        outs = []
        for p in self.outputs[name]:
            ptr = getattr(args[p], "value", args[p])
            t = tensors.get(ptr) if ptr else None
            if t is not None:
                outs.append((p, t, t.clone()))
                _as_bytes(t).fill_(SENTINEL)
        arenas = [m[2] for m in mine]
        bodies = [a.body.clone() if keeps else None for _, _, a, keeps in mine]
        rc = fn(*short)
        _sync(self.device)
        problems = []
        want = REFUSES_WITH.get(name, (ERR_WORKSPACE,))[0]
        if rc != want:
            problems.append("returned %d, not %d, with %d of %d bytes" % (rc, want, short[b], args[b]))
        if any(ptr for ptr in (getattr(args[p], "value", args[p]) for p in self.outputs[name])) and not outs:
            problems.append("none of its output tensors was found: the rig cannot see what it wrote")
        for p, t, saved in outs:
            if not bool((_as_bytes(t) == SENTINEL).all()):
                problems.append("wrote the output at parameter %d" % p)
            t.copy_(saved)
        for a, saved in zip(arenas, bodies):
            if saved is not None and not torch.equal(a.body, saved):
                problems.append("wrote %s" % a.label)
                a.body.copy_(saved)
            r = a.intact()
            if r is not None:
                problems.append("changed guard bytes %d .. %d of %s" % (r[0], r[1], a.label))
                a.mend()
        self.refusals.append((name, region, "; ".join(problems)))

    def short_run(self, case, fill=0x00):
        """R0: one run in which every call that takes a region is first made with `X_bytes - 1`, once per region, its
        outputs pre-filled with a sentinel; then made in full, so that the run goes on.  -> host copies of the outputs;
        self.refusals says what each refused call did."""
        case.reset()
        self.begin_run(fill)
        self.refusals = []
        self._old_tensors = {}
        was = gc.isenabled()
        gc.disable()                                     # tensors made during the run stay in the youngest generation
        try:
            if self.index is not None:
                self._old_tensors = self.index.tensors()
            else:
                _note_tensors(self._old_tensors, gc.get_objects(), self.device)
            self.short = True
            outs = case.run()
        finally:
            self.short = False
            self._old_tensors = {}
            if was:
                gc.enable()
        _sync(self.device)
        return _host(outs)


def _as_bytes(t):
    return t.reshape(-1).view(torch.uint8)


def _note_tensors(found, objects, device):
    """The contiguous tensors on `device` among `objects` into found: {address: the largest that starts there}."""
    device = torch.device(device)
    with warnings.catch_warnings():                      # (looking at every object wakes deprecated module attributes)
        warnings.simplefilter("ignore")
        tensors = [o for o in objects if isinstance(o, torch.Tensor)]
    for o in tensors:
        try:
            if o.device == device and o.numel() and o.is_contiguous() and o.layout == torch.strided:
                ptr = o.data_ptr()
                if ptr not in found or found[ptr].numel() * found[ptr].element_size() < o.numel() * o.element_size():
                    found[ptr] = o
        except Exception:                                # (a tensor subclass without storage)
            pass


# ------------------------------------------------------------------------------------------------ the rig sees: plants
PLANT_BYTES = 1000                                       # no multiple of 256: the upper guard starts unaligned
PlantCase = collections.namedtuple("PlantCase", "inputs poison run reset")


def _plant(device, body_op):
    """A case in plain torch whose run() enters one 1000-byte `workspace` and applies body_op(arena, x) -> output."""
    regs = Regions()
    g = torch.Generator().manual_seed(13)
    x = torch.randn(512, generator=g).to(device)
    p = torch.randn(512, generator=g).to(device)

    def run():
        a = regs.enter("plant", "workspace", PLANT_BYTES, device)
        return [body_op(a, x)]
    return PlantCase([x], [p], run, lambda: None), regs


def plant_write_past(device):
    """Writes one byte past the body (the first byte of the upper guard)."""
    def op(a, x):
        a.body[:8] = 1
        a.high[0] = a.high[0] ^ 0xFF
        return x * 2.0
    return _plant(device, op)


def plant_write_before(device):
    """Writes one byte before the body (the last byte of the lower guard)."""
    def op(a, x):
        a.body[:8] = 1
        a.low[-1] = a.low[-1] ^ 0xFF
        return x * 2.0
    return _plant(device, op)


def plant_reads_stale(device):
    """An output that depends on what the body held: it reads a word of the body it never wrote."""
    def op(a, x):
        stale = a.body[16:20].to(torch.float32).sum()
        a.body[16:20] = (x[:4].abs() * 10).to(torch.uint8)
        return x * 2.0 + stale
    return _plant(device, op)


def plant_well_behaved(device):
    """Writes its scratch before it reads it, inside the body, up to its last byte."""
    def op(a, x):
        a.body[:] = 3
        a.body[-1] = 9
        return x * 2.0 + a.body[-1].to(torch.float32)
    return _plant(device, op)


PLANTS = collections.OrderedDict([("write_past", plant_write_past), ("write_before", plant_write_before),
                                  ("reads_stale", plant_reads_stale), ("well_behaved", plant_well_behaved)])


def judge_plants(device):
    """{plant: Verdict}."""
    out = collections.OrderedDict()
    for name, make in PLANTS.items():
        case, regs = make(device)
        out[name] = judge(case, regs, device)
    return out


def all_changed(v):
    """The (first, last) reports of a verdict over all its runs, as a set."""
    return {r for per in v.changed.values() for r in per.values()}


def any_dirty(v):
    return any(v.dirty.values())
