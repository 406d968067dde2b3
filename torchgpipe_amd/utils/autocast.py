"""The calling thread's autocast state, captured once and re-entered elsewhere.

Autocast state is thread-local, and a pipeline runs a micro-batch's forward, its
recomputation and its captured graphs on other threads (device workers, the autograd
engine, the backward helper, the big-stack worker) and at other times (``backward()``
after the ``with torch.autocast(...)`` block) than the user's call.  Everything that has
to carry the state there uses this one helper: :func:`capture` on the thread and at the
moment that define it, ``state.entered()`` around the code that must see it.

The state is the enabled flag and dtype for ``'cuda'`` and ``'cpu'``, and the weight-cast
cache flag.  A disabled device type is re-entered as disabled, so an inner
``torch.autocast(..., enabled=False)`` wins wherever the state is carried to.
"""
import contextlib
from typing import Any, ContextManager, Hashable, List, Optional, Tuple

import torch

__all__ = ['AutocastState', 'capture']

KINDS = ('cuda', 'cpu')

_NULL: ContextManager[None] = contextlib.nullcontext()


def _current() -> Tuple[Any, ...]:
    return tuple((torch.is_autocast_enabled(kind), torch.get_autocast_dtype(kind))
                 for kind in KINDS) + (torch.is_autocast_cache_enabled(),)


class AutocastState:
    """An immutable snapshot: ``key`` is hashable (for caches keyed on the step's mode)."""

    __slots__ = ('key',)

    def __init__(self, key: Tuple[Any, ...]) -> None:
        self.key: Hashable = key

    @property
    def any_enabled(self) -> bool:
        return any(enabled for enabled, _ in self.key[:len(KINDS)])  # type: ignore[index]

    def entered(self, cache: Optional[bool] = None) -> ContextManager[None]:
        """A context under which the current thread has this state (nothing to enter when
        it has it already, the common case outside autocast).  ``cache`` overrides the
        weight-cast cache flag: a graph capture passes ``False``, since a cast cached by
        one capture would be read, never recomputed, by the next graph's replays, and one
        cached under ``no_grad`` carries no graph.  Without autocast there is no cast to
        cache and the flag is left alone."""
        key: Tuple[Any, ...] = self.key  # type: ignore[assignment]
        if cache is not None and self.any_enabled:
            key = key[:-1] + (cache,)
        if _current() == key:
            return _NULL
        return self._enter(key)

    @staticmethod
    @contextlib.contextmanager
    def _enter(key: Tuple[Any, ...]) -> Any:
        *per_kind, cache = key
        with contextlib.ExitStack() as stack:
            for kind, (enabled, dtype) in zip(KINDS, per_kind):
                stack.enter_context(torch.autocast(kind, dtype=dtype, enabled=enabled,
                                                   cache_enabled=cache))
            yield

    def __eq__(self, other: object) -> bool:
        return isinstance(other, AutocastState) and other.key == self.key

    def __hash__(self) -> int:
        return hash(self.key)

    def __repr__(self) -> str:
        parts: List[str] = [f'{kind}={dtype}' for kind, (enabled, dtype)
                            in zip(KINDS, self.key[:len(KINDS)])  # type: ignore[index]
                            if enabled]
        return f'AutocastState({", ".join(parts) or "off"})'


def capture() -> AutocastState:
    """The current thread's autocast state."""
    return AutocastState(_current())

