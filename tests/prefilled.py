"""Adverse starts for memory the library does not own: every ``torch.empty`` tensor a call hands it (workspaces, outputs) and the scratch a
module caches per stream.  A result must not depend on what that memory held before (include/mdgat_hip.h: "a workspace and every output
buffer may hold anything on entry"), so the GPU tests run the same call under different fills and compare bits.

``prefilled(mode)``     wraps torch.empty / empty_like / empty_strided / Tensor.new_empty for its duration and fills what they return
``refill_cached``       fills the scratch tensors a module keeps (``_DeviceState.workspaces``)
``spy``                 counts the calls of ctypes entries, so a case can assert that the C entry it claims to cover really ran
``same_bits``           bit equality of two (nests of) tensors, NaN payloads and signed zeros included"""
import contextlib

import torch

MODES = ('zero', 'ones', 'replay')
_FILL = {'zero': 0x00, 'ones': 0xFF}
_WRAPPED = ((torch, 'empty'), (torch, 'empty_like'), (torch, 'empty_strided'), (torch.Tensor, 'new_empty'))


class Prefill:
    """What one ``prefilled`` context saw.  ``count`` / ``bytes``: allocations it filled and their storage bytes; ``scratch_bytes``: the
    largest uint8 allocation among them (every workspace of the package is one uint8 tensor); ``replayed``: allocations a 'replay' context
    started from recorded bytes (the others fell back to 0xFF); ``final``: with ``record=True``, after exit, per allocation in order
    (shape, dtype, the storage's last bytes as a uint8 tensor)."""

    def __init__(self, mode, source, record):
        self.mode, self.source, self.record = mode, source, record
        self.count = self.bytes = self.scratch_bytes = self.replayed = 0
        self.final = None
        self._live = []             # (shape, dtype, uint8 view of the storage): kept alive until exit, where ``final`` is read

    def saw_scratch(self, nbytes) -> bool:
        """Was a uint8 allocation of at least ``nbytes`` filled - did the fill reach a workspace of that size?"""
        return self.scratch_bytes >= int(nbytes)


def _capturing(t):
    return t.is_cuda and torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


@contextlib.contextmanager
def prefilled(mode, source=None, record=False, touch=None):
    """Every tensor the four allocation functions return inside the context starts with known bytes: 'zero' 0x00, 'ones' 0xFF (floats NaN,
    flags and epochs all-ones, integers -1), 'replay' the final bytes of the same-numbered allocation of ``source`` - a ``Prefill`` of an
    earlier context run with ``record=True`` - where shape, dtype and storage size agree, 0xFF otherwise.  Only device tensors are touched
    (``touch``: another predicate, for the helper's own CPU tests), none while the current stream is capturing.  The functions are put
    back on exit, after an exception too.  Yields the context's ``Prefill``."""
    if mode not in MODES:
        raise ValueError(f'mode {mode!r}: expected one of {MODES}')
    if (mode == 'replay') != (source is not None):
        raise ValueError("'replay' needs source= (a recorded Prefill), the other modes take none")
    if source is not None and source.final is None:
        raise ValueError('source= was not recorded (prefilled(..., record=True)) or its context is still open')
    touch = touch or (lambda t: t.is_cuda)
    originals = [(owner, name, getattr(owner, name)) for owner, name in _WRAPPED]
    raw_empty = originals[0][2]
    state = Prefill(mode, source, record)

    def fill(t):
        if not isinstance(t, torch.Tensor) or not touch(t) or _capturing(t):
            return t
        storage = t.untyped_storage()
        nbytes = storage.nbytes()
        if nbytes == 0:             # nothing to fill: not counted, so the numbering of a replay does not depend on it
            return t
        k = state.count
        state.count += 1
        flat = raw_empty(0, dtype=torch.uint8, device=t.device).set_(storage)
        old = source.final[k] if mode == 'replay' and k < len(source.final) else None
        if old is not None and old[0] == tuple(t.shape) and old[1] == t.dtype and old[2].numel() == nbytes:
            flat.copy_(old[2])
            state.replayed += 1
        else:
            flat.fill_(_FILL.get(mode, 0xFF))
        state.bytes += nbytes
        if t.dtype == torch.uint8:
            state.scratch_bytes = max(state.scratch_bytes, nbytes)
        if record:
            state._live.append((tuple(t.shape), t.dtype, flat))
        return t

    def wrap(fn):
        def wrapped(*args, **kwargs):
            return fill(fn(*args, **kwargs))
        wrapped.__wrapped__ = fn
        return wrapped

    try:
        for owner, name, fn in originals:
            setattr(owner, name, wrap(fn))
        yield state
    finally:
        for owner, name, fn in originals:
            setattr(owner, name, fn)
        if record:
            if torch.cuda.is_available() and any(f.is_cuda for _, _, f in state._live):
                torch.cuda.synchronize()
            state.final = [(shape, dtype, f.clone()) for shape, dtype, f in state._live]
        state._live = []


def refill_cached(net, device, byte):
    """Fill every scratch tensor ``net`` keeps for ``device`` (one per stream it ran on) with ``byte``; returns the bytes filled.  The
    device is synchronised first: nothing in flight reads the scratch."""
    device = torch.device(device)
    st = net._state_for(device)
    torch.cuda.synchronize(device)
    total = 0
    with st.lock:
        for ws in st.workspaces.values():
            ws.fill_(int(byte))
            total += ws.numel()
    torch.cuda.synchronize(device)
    return total


class Spy:
    """``calls[name]``: calls of the entry so far; ``returned[name]``: the largest integer it returned (a ``*_workspace_bytes`` query:
    the most it asked for)."""

    def __init__(self, names):
        self.calls = {n: 0 for n in names}
        self.returned = {n: 0 for n in names}

    def forget_sizes(self):
        """start a new call: ``most_asked`` then speaks of the queries made from here on"""
        for n in self.returned:
            self.returned[n] = 0

    def most_asked(self) -> int:
        """the largest size a spied ``*_workspace_bytes`` query returned"""
        return max([v for n, v in self.returned.items() if n.endswith('workspace_bytes')] + [0])


@contextlib.contextmanager
def spy(lib, names):
    """Count the calls of the ctypes entries ``names`` of ``lib`` (the loaded CDLL, or any object whose attributes are callables) for the
    context's duration; the entries are put back on exit.  Yields a ``Spy``."""
    names = tuple(names)
    s = Spy(names)
    originals = {n: getattr(lib, n) for n in names}

    def wrap(name, fn):
        def wrapped(*args):
            s.calls[name] += 1
            r = fn(*args)
            if isinstance(r, int):
                s.returned[name] = max(s.returned[name], r)
            return r
        return wrapped

    try:
        for n, fn in originals.items():
            setattr(lib, n, wrap(n, fn))
        yield s
    finally:
        for n, fn in originals.items():
            setattr(lib, n, fn)


def leaves(x, path=''):
    """(path, tensor) for every tensor in a nest of tuples, lists and dicts; other leaves (None, numbers, strings) are skipped."""
    if isinstance(x, torch.Tensor):
        yield path, x
    elif isinstance(x, dict):
        for k in x:
            yield from leaves(x[k], f'{path}[{k!r}]')
    elif isinstance(x, (tuple, list)):
        for i, v in enumerate(x):
            yield from leaves(v, f'{path}[{i}]')


def snapshot(x):
    """The tensors of a nest as independent contiguous copies (a later call cannot reuse their memory under the comparison)."""
    return [(p, t.detach().clone(memory_format=torch.contiguous_format)) for p, t in leaves(x)]


def same_bits(a, b, what=''):
    """Assert that two snapshots hold the same tensors bit for bit (shape, dtype and every byte: NaN equals NaN, -0.0 differs from 0.0)."""
    assert [p for p, _ in a] == [p for p, _ in b], f'{what}: the calls returned different structures'
    for (p, x), (_, y) in zip(a, b):
        assert x.shape == y.shape and x.dtype == y.dtype, f'{what}: {p}: {tuple(x.shape)} {x.dtype} against {tuple(y.shape)} {y.dtype}'
        bx, by = (t.reshape(-1).view(torch.uint8) if t.dtype != torch.bool else t.reshape(-1).to(torch.uint8) for t in (x, y))
        if not torch.equal(bx, by):
            item = max(x.element_size(), 1)
            first = int((bx != by).nonzero()[0]) // item
            n_bad = int((bx.reshape(-1, item) != by.reshape(-1, item)).any(dim=1).sum())
            raise AssertionError(f'{what}: {p}: {n_bad} of {x.numel()} elements differ, the first at flat index {first}: '
                                 f'{x.reshape(-1)[first].item()!r} against {y.reshape(-1)[first].item()!r}')
