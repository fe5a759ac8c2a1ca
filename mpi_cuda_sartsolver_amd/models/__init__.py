"""Solvers and problem data: RTM shard, Laplacian, GPU/CPU SART engines, fp64 oracles."""

_HOLDOUT = ("holdout_sums", "solve_holdout")


def __getattr__(name):  # the hold-out study's entry points, loaded on first use (they bring torch and the kernels)
    if name in _HOLDOUT:
        from . import holdout

        return getattr(holdout, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def __dir__():
    return sorted(list(globals()) + list(_HOLDOUT))
