"""The macr_shard_* calls of a mode ("plain", "det", "inv") with a host address standing in for every buffer, for the CPU tests of
their refusals (tests/test_shard_deterministic_cpu.py, tests/test_shard_invariant_cpu.py): argument validation comes before any
device work, so the pointers handed in are never dereferenced."""
import ctypes

B, D = 300, 64


def aligned_mem():
    """a 256-byte aligned host address standing in for every buffer: (the buffer that keeps it alive, the address)"""
    buf = ctypes.create_string_buffer(8192)
    return buf, ctypes.c_void_p((ctypes.addressof(buf) + 255) & ~255)


def _hyper(lib, **over):
    a = dict(lr=1e-3, beta1=0.9, beta2=0.999, adam_eps=1e-8, decay=1e-5, alpha=1e-2, beta=1e-3, batch_size_cfg=1024)
    a.update(over)
    return lib.Hyper(*[a[n] for n, _ in lib.Hyper._fields_])


def entry(lib, base, mode):
    """macr_shard_<base> of a mode (every call below has a twin in every mode it is asked for)"""
    return getattr(lib.lib(), "macr_shard_" + base + {"plain": "", "det": "_det", "inv": "_inv"}[mode])


def backward(lib, mem, mode, kind=None, ws_bytes=1 << 30, rows3="p", hp=None):
    p = mem[1]
    hp = hp or _hyper(lib)
    return entry(lib, "backward", mode)(lib.LOSS_RUBIBCEBOTH if kind is None else kind, B, D, p if rows3 == "p" else None, p, p, p,
                                        ctypes.byref(hp), p, None, None, p, ws_bytes, None)


def forward_slice(lib, mem, mode, kind=None, ws_bytes=1 << 30, t0=32, n=64, w="p", b=B, d=D):
    p = mem[1]
    return entry(lib, "forward_slice", mode)(lib.LOSS_RUBIBCEBOTH if kind is None else kind, b, d, t0, n, p, p if w == "p" else None, p,
                                             None, None, p, ws_bytes, None)


def backward_slice(lib, mem, mode, kind=None, ws_bytes=1 << 30, t0=32, n=64, w="p", b=B, d=D):
    p = mem[1]
    hp = _hyper(lib)
    return entry(lib, "backward_slice", mode)(lib.LOSS_RUBIBCEBOTH if kind is None else kind, b, d, t0, n, p, p if w == "p" else None, p,
                                              p, ctypes.byref(hp), p, p, None, None, p, ws_bytes, None)


def apply(lib, mem, form, ws_bytes=1 << 30, u="p", lazy_period=4, n_users_loc=40):
    """form: "plain" (macr_shard_apply), "lazy" (macr_shard_apply_lazy); "det" / "inv" (lazy = NULL), "det_lazy" / "inv_lazy" """
    p, L = mem[1], lib.lib()
    hp = _hyper(lib)
    lz = lib.LazyAdam(p, p, p, lazy_period)
    head = [lib.LOSS_RUBIBCEBOTH, B, D, n_users_loc, 50, 0, 1, 0, 1, p if u == "p" else None, p, p] + [p] * 16 + [ctypes.byref(hp)]
    tail = [p, ws_bytes, None]
    if form == "plain":
        return L.macr_shard_apply(*(head + tail))
    if form == "lazy":
        return L.macr_shard_apply_lazy(*(head + [ctypes.byref(lz)] + tail))
    return entry(lib, "apply", form[:3])(*(head + [ctypes.byref(lz) if form.endswith("_lazy") else None] + tail))
