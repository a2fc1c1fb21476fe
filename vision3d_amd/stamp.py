"""A value derived from tensors is stored with the stamp of those tensors; a capture stores the stamps of what it baked in.
A stamp is (data_ptr, _version) per tensor: every in-place update bumps the version (optimizer steps, load_state_dict), a Parameter
replaced on its module (.cuda(), load_state_dict(assign=True)) has another pointer.  Comparing stamps costs no device work."""


def stamp_of(tensors, *extra):
    """Any iterable of tensors (None is skipped) -> a tuple that differs once one of them changed; `extra` is appended as it is."""
    return tuple((t.data_ptr(), t._version) for t in tensors if t is not None) + extra


def cached(owner, slot, tensors, build, key=None, extra=()):
    """`build()`'s value, rebuilt only when the stamp of `tensors` (+ extra) moved.  owner.__dict__[slot] = {key: (stamp, value)}: in
    __dict__, not an attribute, so nn.Module.__setattr__ / __getattr__ and state_dict stay out of it."""
    cache, stamp = owner.__dict__.setdefault(slot, {}), stamp_of(tensors, *extra)
    hit = cache.get(key)
    if hit is None or hit[0] != stamp:
        hit = cache[key] = (stamp, build())
    return hit[1]
