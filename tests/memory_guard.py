"""Memory that behaves like production memory at its worst, for tests/test_memory_contract.py (a helper, not a test).

`guarded_workspaces(fill)` hands every `_C.workspace` request an exact-size payload, pre-filled with `fill`, between two
guard bands that are checked when the context ends.  `dirty_allocator(fill)` leaves the caching allocator's free memory
holding `fill`, so the `torch.empty` outputs of the wrappers start from it instead of from zeros."""
import contextlib
import weakref

GUARD = 0x5A                        # the guard byte: differs from every payload fill
FILLS = (0x00, 0xA5, 0xFF)          # zeros (the baseline); small negative float / large negative int / in-range id; NaN / -1
MIN_BAND = 64 << 10                 # each guard band is at least this long ...
MAX_BAND = 8 << 20                  # ... at least as long as the payload, and at most this long
ALIGN = 256                         # the payload starts at a multiple of this (entries ask for 16-byte alignment)

# dirty_allocator: what is filled and freed.  torch serves requests of up to 1 MiB from 2 MiB blocks of a small pool and
# larger ones from a large pool; a request takes the smallest free piece that holds it, so the leftover pieces of blocks
# that live tensors still pin have to be soaked up by size class before fresh blocks are dirtied.
SMALL_SIZES = (1 << 20, 256 << 10, 64 << 10, 16 << 10, 4 << 10, 512)   # descending: each class soaks up the pieces it fits
SMALL_COUNT = 16                    # per class; 16 x 1 MiB alone is eight small-pool blocks
LARGE_SIZES = (8 << 20, 2 << 20)    # soak up the pieces left in 20 MiB large-pool blocks (requests below 10 MiB)
LARGE_COUNT = 6                     # per class: more than two 20 MiB blocks' worth of 8 MiB requests
LARGE_ONE = 96 << 20                # one tensor larger than any output of a case here (the largest is under 40 MiB)
PROBES = (4 << 10, 2 << 20)         # a fresh small-pool and a fresh large-pool request must both read back as `fill`


def layout(nbytes):
    """(front, n, back) of the arena for one request: payload bytes [front, front + n), guard bands on both sides."""
    n = max(int(nbytes), 16)
    band = min(max(MIN_BAND, n), MAX_BAND)
    front = (band + ALIGN - 1) // ALIGN * ALIGN
    return front, n, band


def first_damage(band):
    """Index of the first byte of a guard band (a device uint8 tensor) that is no longer GUARD, or None."""
    bad = band != GUARD
    if not bool(bad.any()):
        return None
    return int(bad.nonzero()[0, 0])


class Guarded(object):
    """What `guarded_workspaces` yields: `requests` counts the workspaces handed out; `arenas` keeps them alive.
    With `reuse`, the first payload is handed out again only once the view handed out before has been dropped: two
    workspaces that an entry holds at the same time are never the same memory."""

    def __init__(self, fill, reuse):
        self.fill, self.reuse = int(fill), reuse
        self.arenas = []                                   # (arena, front, n)
        self.requests = 0
        self.lent = None                                   # reuse: weak reference to the view of arenas[0] last handed out

    def take(self, nbytes, device):
        import torch
        front, n, back = layout(nbytes)
        self.requests += 1
        if self.reuse and self.arenas and self.arenas[0][2] >= n and (self.lent is None or self.lent() is None):
            arena, f0, _ = self.arenas[0]
            view = arena[f0:f0 + n]                        # the first payload again, as it was left
            self.lent = weakref.ref(view)
            return view
        arena = torch.full((front + n + back,), GUARD, dtype=torch.uint8, device=device)
        arena[front:front + n] = self.fill
        self.arenas.append((arena, front, n))
        view = arena[front:front + n]
        if len(self.arenas) == 1:
            self.lent = weakref.ref(view)
        return view

    def damage(self):
        """One line per damaged guard band: the request's size and the first damaged offset relative to the payload."""
        found = []
        for k, (arena, front, n) in enumerate(self.arenas):
            at = first_damage(arena[front + n:])
            if at is not None:
                found.append("request %d of %d bytes: byte %d of the payload's range (%d past its end) was written"
                             % (k, n, n + at, at))
            bad = arena[:front] != GUARD
            if bool(bad.any()):
                at = int(bad.nonzero()[-1, 0])             # the damaged byte nearest the payload
                found.append("request %d of %d bytes: byte %d (before the payload's start) was written"
                             % (k, n, at - front))
        return found


@contextlib.contextmanager
def guarded_workspaces(fill, reuse=False):
    """Replace `_C.workspace` by exact-size, guard-banded, `fill`-ed payloads; check the guards on the way out.
    `reuse`: a request that fits the first payload gets that payload again, unfilled (a block the allocator hands back)."""
    import torch
    from centerpoly_amd import _C
    state = Guarded(fill, reuse)
    original = _C.workspace
    _C.workspace = state.take
    try:
        try:
            yield state
        except Exception as failure:
            # the body failed first: read the guards all the same, so that an overrun which also spoiled a result is
            # reported with its offset and not only as a wrong value
            found = _damage_after_failure(state)
            if found:
                raise AssertionError("%s: %s\nand guard bytes damaged: %s"
                                     % (type(failure).__name__, failure, "; ".join(found))) from failure
            raise
        torch.cuda.synchronize()
        found = state.damage()
        assert not found, "guard bytes damaged: " + "; ".join(found)
    finally:
        _C.workspace = original
        state.arenas = []


def _damage_after_failure(state):
    """The damaged guard bands after the body raised; nothing when the device itself no longer answers."""
    import torch
    try:
        torch.cuda.synchronize()
        return state.damage()
    except RuntimeError:
        return []


def dirty_allocator(fill):
    """Leave the allocator's free memory holding `fill` and prove it: fresh `torch.empty` requests read back as `fill`."""
    import torch
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    held = []
    for size in SMALL_SIZES:
        held += [torch.full((size,), int(fill), dtype=torch.uint8, device="cuda") for _ in range(SMALL_COUNT)]
    for size in LARGE_SIZES:
        held += [torch.full((size,), int(fill), dtype=torch.uint8, device="cuda") for _ in range(LARGE_COUNT)]
    held.append(torch.full((LARGE_ONE,), int(fill), dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
    del held
    for size in PROBES:
        probe = torch.empty(size, dtype=torch.uint8, device="cuda")
        live = bool((probe == int(fill)).all())
        del probe
        assert live, "a fresh torch.empty of %d bytes does not read back as 0x%02X: the allocator is not polluted" \
            % (size, fill)


def clean_allocator():
    """Hand the polluted blocks back to the driver, so that the tests that run afterwards get the memory they always got."""
    import torch
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
