"""Prepared forms of weights for the inference kernels -- the split-bf16, fragment-ordered copies of
cp_conv_mfma_prepare / cp_conv7x7_c3_prepare / cp_heads_fused_prepare_w2 and the DCN workspaces whose head holds them
-- cached on the module that launches them, so that the permutation runs once instead of on every call.

One rule for when a form is still valid: every source tensor is the same object with the same `_version`, storage,
device and shape.  The version alone is not enough: `param.data = t`, `module.to(...)` and parameter flattening point
a tensor at new storage without bumping it."""

ATTR = "_prepared"          # the one dict attribute that holds an owner's slots: slot -> (key, tensors, value)


def stamp(t):
    """What a form prepared from `t` stays valid for: the object, its in-place version, storage, device and shape."""
    return id(t), t._version, t.data_ptr(), t.device, t.shape


def prepared(owner, slot, tensors, build, extra=()):
    """(value, built_now): the value kept on `owner` under `slot` while `tensors` and `extra` are unchanged; otherwise
    build() -- its result is stored and built_now is True.  (The entry holds `tensors` themselves, so no id in its key
    can be reused while it lives.)"""
    slots = owner.__dict__.get(ATTR)
    if slots is None:
        slots = owner.__dict__[ATTR] = {}
    key = (extra, *map(stamp, tensors))
    entry = slots.get(slot)
    if entry is not None and entry[0] == key:
        return entry[2], False
    value = build()
    slots[slot] = (key, tensors, value)
    return value, True


def release_prepared(module):
    """Drop the prepared forms of `module` and of every submodule."""
    for m in module.modules():
        m.__dict__.pop(ATTR, None)


def release_inference(net):
    """Undo prepare_inference() on `net` (train() calls it): the prepared forms, and the folded BatchNorm weights
    (`_folded`), concatenated heads (`_heads_cat`) and folded inter-stack convolutions (`_inter_folded`) they were
    made from."""
    release_prepared(net)
    for m in net.modules():
        for name in ("_folded", "_heads_cat", "_inter_folded"):
            if name in m.__dict__:
                m.__dict__[name] = None
