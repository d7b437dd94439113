"""Fragment plan and schedule of Streaming DiLoCo (Douillard et al., 2025; docs/DESIGN.md §4).

The model is cut into ``P`` fragments of whole decoder layers.  Each fragment is synchronised every ``H`` inner
steps, the fragments at staggered offsets, so the peak of the outer communication is 1/P of the monolithic
burst.  A fragment is a short list of spans ``[start, end)`` of the flat :class:`ParamStore` vector:

* layer ``i`` spans from the offset of its first parameter to the offset of layer ``i+1``'s first parameter
  (padding included: every layer starts on a 64-element boundary, so every span boundary is 64-aligned);
* ``strided`` (the paper's choice): fragment ``p`` owns layers ``p, p+P, p+2P, ...``; ``sequential``: a contiguous
  run of ``ceil`` / ``floor(L/P)`` layers;
* ``model.embed_tokens`` joins the fragment of layer 0; ``model.norm``, an untied ``lm_head`` and the trailing
  padding of the flat vector join the fragment of layer ``L-1``;
* adjacent spans of one fragment are merged, and the fragments partition ``[0, store.numel)`` exactly once.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

Span = Tuple[int, int]
PATTERNS = ("strided", "sequential")


def layer_owner(num_layers: int, P: int, pattern: str = "strided") -> List[int]:
    """Fragment index of every decoder layer."""
    if pattern not in PATTERNS:
        raise ValueError(f"fragment pattern must be one of {PATTERNS}, not {pattern!r}")
    if not 1 <= P <= num_layers:
        raise ValueError(f"fragments must be in [1, num_layers={num_layers}], got {P}")
    if pattern == "strided":
        return [i % P for i in range(num_layers)]
    q, r = divmod(num_layers, P)  # the first r fragments own ceil(L/P) layers, the others floor(L/P)
    owner = []
    for p in range(P):
        owner += [p] * (q + (1 if p < r else 0))
    return owner


def plan_fragments(store, num_layers: int, P: int, pattern: str = "strided") -> List[List[Span]]:
    """Spans of every fragment, in elements of the flat vector of ``store`` (see the module doc)."""
    owner = layer_owner(num_layers, P, pattern)
    first = [store.offsets[next(n for n in store.names if n.startswith(f"model.layers.{i}."))]
             for i in range(num_layers)]
    tail = store.offsets["model.norm.weight"]
    bounds = first + [tail]
    pieces = [(0, first[0], owner[0])]  # embedding
    pieces += [(bounds[i], bounds[i + 1], owner[i]) for i in range(num_layers)]
    pieces.append((tail, store.numel, owner[-1]))  # final norm, untied lm_head, trailing padding
    frags: List[List[Span]] = [[] for _ in range(P)]
    for a, b, p in pieces:
        if a % 64 or b % 64 or b < a:
            raise ValueError(f"fragment span [{a}, {b}) is not 64-aligned: the flat layout must align every layer")
        if b == a:
            continue
        if frags[p] and frags[p][-1][1] == a:
            frags[p][-1] = (frags[p][-1][0], b)
        else:
            frags[p].append((a, b))
    return frags


def fragment_due(t: int, H: int, P: int) -> Optional[int]:
    """The fragment sent after inner step ``t`` (1-based), or None: fragment ``p`` goes when
    ``t % H == ((p+1)*H // P) % H``, i.e. in every round the fragments go in order 0..P-1 at
    ``H/P, 2H/P, ..., H`` (distinct steps, since P <= H)."""
    for p in range(P):
        if t % H == ((p + 1) * H // P) % H:
            return p
    return None
