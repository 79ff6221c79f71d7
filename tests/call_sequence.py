"""The order in which tests/test_call_sequence_gpu.py interleaves its configurations: a seeded closed walk over the complete directed
graph on the names, so that every ordered pair X -> Y with X != Y is a pair of consecutive calls exactly once (n (n - 1) + 1 calls:
the shortest sequence that can hold them all). Hierholzer's algorithm on a shuffled adjacency; plain Python, checked on the CPU."""
import random


def ordered_pairs(seq):
    return set(zip(seq[:-1], seq[1:]))


def covers_every_ordered_pair(seq, names):
    want = {(x, y) for x in names for y in names if x != y}
    return want <= ordered_pairs(seq) and all(x != y for x, y in zip(seq[:-1], seq[1:]))


def sequence(names, seed=0):
    names = list(names)
    assert len(set(names)) == len(names) >= 2
    rng = random.Random(seed)
    out_edges = {x: [y for y in names if y != x] for x in names}
    for v in out_edges.values():
        rng.shuffle(v)
    stack, walk = [names[rng.randrange(len(names))]], []
    while stack:                                        # every vertex has in-degree = out-degree: an Eulerian circuit exists
        v = stack[-1]
        if out_edges[v]:
            stack.append(out_edges[v].pop())
        else:
            walk.append(stack.pop())
    walk.reverse()
    assert len(walk) == len(names) * (len(names) - 1) + 1 and covers_every_ordered_pair(walk, names)
    return walk
