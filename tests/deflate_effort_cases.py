"""Inputs for the high effort of the device DEFLATE: the smallest at which each of its rules can go wrong.  Every case is
(name, data, bpp, row) like those of deflate_cases, built for a sub-step of `substep` positions and chains of `probes`
entries, and comes with `marks`: the positions the case is about.  tests/test_deflate_effort_cpu.py proves on the model,
without a GPU, that each case reaches its edge.  Noise is drawn so that no 4-byte group outside the planted pieces shares a
hash bucket with a group inside them (deflate_cases._avoiding_noise): the chains hold exactly what the case planted.
Test harness only."""
import numpy as np

import deflate_cases as C

CHUNK = 65535
PIECE, TAIL = 24, 20  # bytes of a planted marker, of the continuation that tells its occurrences apart


class _Builder:
    """Pieces are drawn and placed first; the noise between them is drawn when the stream is built, against the buckets of
    every piece."""

    def __init__(self, seed):
        self.rng = np.random.RandomState(seed)
        self.own = set()  # buckets of the planted groups
        self.plan = []

    def piece(self, n):
        """n planted bytes whose groups have a bucket each, unknown to the noise."""
        return C._avoiding_noise(n, self.rng, set(), fresh=self.own)

    def put(self, at, *pieces):
        self.plan.append((at, b"".join(pieces)))

    def build(self, end=None):
        d = bytearray()
        for at, text in sorted(self.plan) + ([(end, b"")] if end else []):
            assert at >= len(d), "the case's pieces overlap"
            if at > len(d):
                d += C._avoiding_noise(at - len(d), self.rng, self.own, tail=bytes(d))
            d += text
        return bytes(d)


def _differing(tails):
    """Continuations that differ from each other in their first byte."""
    for i, t in enumerate(tails):
        t = bytearray(t)
        t[0] = (2 * i + 1) & 255
        tails[i] = bytes(t)
    return tails


def _chain_depth(substep, probes):
    """Three groups of marker occurrences, one occurrence per sub-step.  The last occurrence of each group goes on as the
    2nd, the `probes`-th and the `probes + 1`-th earlier occurrence did, every other earlier occurrence differently: the
    first two are found through the chain at that depth, the third is one entry too deep and the nearest wins the tie."""
    b = _Builder(31)
    marks, at, step = {}, 2 * substep, substep + PIECE + TAIL + 8
    for name, count, target in (("second", 3, 2), ("kth", probes + 1, probes), ("beyond", probes + 2, probes + 1)):
        marker = b.piece(PIECE)
        tails = _differing([b.piece(TAIL) for _ in range(count)])
        starts = []
        for i in range(count):  # occurrence i is entry count - i of the final one's chain
            b.put(at, marker, tails[i])
            starts.append(at)
            at += step
        b.put(at, marker, tails[count - target], bytes([254]))
        marks[name] = dict(at=at, depth=target, source=starts[count - target], nearest=starts[-1])
        at += step
    return b.build(at), 0, 0, marks


def _visibility(substep, probes):
    """The same marker twice inside one sub-step (the second must not find the first: literals), and twice with a sub-step
    boundary between them (a match)."""
    b = _Builder(32)
    gap = 4
    marker = b.piece(PIECE)
    inside = 5 * substep + 2  # both copies in [5 * substep, 6 * substep)
    b.put(inside, marker)
    b.put(inside + PIECE + gap, marker)
    assert PIECE + gap + PIECE + 2 <= substep
    other = b.piece(PIECE)
    across = 9 * substep  # the second copy starts a sub-step
    b.put(across - PIECE - gap, other)
    b.put(across, other)
    return b.build(across + PIECE + 3 * substep), 0, 0, dict(inside=inside + PIECE + gap, across=across, dist=PIECE + gap)


def _lazy(substep, probes):
    """Three places where a match of some length at p meets a match at p + 1: a strictly longer one (p becomes a literal),
    an equally long one (p keeps its match), and a strictly longer one that ends with the chunk."""
    b = _Builder(33)
    at = 3 * substep
    plan = []
    for name, here, there in (("defer", 5, 9), ("tie", 6, 6), ("end", 4, 7)):
        text = b.piece(1 + max(here - 1, there))  # x, then what follows it
        b.put(at, text[:here], bytes([250]))  # x and here - 1 more, then something else
        at += 2 * substep
        b.put(at, text[1:1 + there], bytes([252]))  # the same without x, `there` long
        at += 2 * substep
        plan.append((name, text, here, there))
    marks = {}
    for name, text, here, there in plan:
        b.put(at, text)
        marks[name] = dict(at=at, here=here, there=there)
        if name != "end":
            b.put(at + len(text), bytes([248]))
            at += 2 * substep
    data = b.build()
    assert marks["end"]["at"] + 1 + marks["end"]["there"] == len(data)  # the longer match ends with the stream
    return data, 0, 0, marks


def _window_chain(substep, probes):
    """Second chunk: a marker whose chain runs into the window in front of the chunk — an occurrence 2,000 back, one
    exactly 32,768 back that goes on for longer (the winner), and one 300 farther that goes on for longest and must not
    be looked at."""
    b = _Builder(34)
    marker = b.piece(PIECE)
    tails = _differing([b.piece(TAIL) for _ in range(3)])
    longest = tails[0] + b.piece(TAIL)
    at = CHUNK + 1000
    b.put(at - WINDOW_D - 300, marker, longest)
    b.put(at - WINDOW_D, marker, tails[0], bytes([254]))
    b.put(at - 2000, marker, tails[1])
    b.put(at, marker, longest)
    return b.build(at + 1500), 0, 0, dict(at=at)


WINDOW_D = 32768


def _collision(substep, probes):
    """The nearest entry of a chain is another 4-byte group in the same bucket (no byte agrees); the match lies behind it."""
    b = _Builder(35)
    marker = b.piece(PIECE)
    want = C._bucket(*marker[:4])
    rng = np.random.RandomState(36)
    while True:
        g = bytes(int(v) * 2 + 1 for v in rng.randint(0, 128, 4))
        if g[0] != marker[0] and C._bucket(*g) == want:
            break
    at = 3 * substep
    b.put(at, marker)
    collide, final = at + 2 * substep, at + 5 * substep
    b.put(collide, g)
    b.put(final, marker)
    return b.build(final + 2 * substep), 0, 0, dict(at=final, collide=collide, source=at)


_BUILDERS = {"chain_depth": _chain_depth, "visibility": _visibility, "lazy": _lazy, "window_chain": _window_chain,
             "collision": _collision}
OWN = list(_BUILDERS)
REUSED = ["gradient_row", "flat_row", "tiny_7", "substep_1025", "chunk_%d" % (CHUNK + 1027)]  # of deflate_cases
NAMES = OWN + REUSED
_CACHE, _MODEL = {}, {}


def get(name, substep, probes):
    """-> (name, data, bpp, row, marks), built once"""
    key = (name, substep, probes)
    if key not in _CACHE:
        if name in _BUILDERS:
            data, bpp, row, marks = _BUILDERS[name](substep, probes)
        else:
            _, data, bpp, row = C.get(name)
            marks = {}
        _CACHE[key] = (name, data, bpp, row, marks)
    return _CACHE[key]


def model(name, substep, probes):
    """-> (token lists per chunk of the model, its trace per chunk), computed once and shared"""
    key = (name, substep, probes)
    if key not in _MODEL:
        import deflate_effort_model as M
        _, data, bpp, row, _ = get(name, substep, probes)
        trace = []
        _MODEL[key] = (M.effort_model(data, bpp, row, substep, probes, trace), trace)
    return _MODEL[key]
