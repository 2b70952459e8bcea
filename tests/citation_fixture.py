"""A seeded writer of a small directory in the Planetoid file layout (ind.<kind>.{x,y,tx,ty,allx,ally,graph} + ind.<kind>.test.index),
the layout tasks/citation_network_task.py of the reference reads.  tests/golden/make_reference_run_citation.py ran the reference's
own loader over exactly these directories; the tests write them again (same seed, same bytes in every array) and load them with the
package's loader.

kind "cora":     560 allx rows of which the first 40 are labelled (x, y), 100 test rows whose ids 560..659 appear in test.index in a
                 shuffled order; 48 bag-of-words features at ~8 % density, a few all-zero feature rows (their row sum is 0: the
                 reciprocal must count as 0); 5 classes; neighbour lists with duplicates, self references and empty lists; the graph
                 dict's keys are NOT in ascending order (edge order follows the dict's iteration order).     -> V = 660
kind "citeseer": the same, but test.index names 100 ids out of 560..666: 7 ids of that range have no row in tx / ty (isolated nodes
                 the files leave out; the loader gives them zero features and zero label rows = class 0), the first id behind
                 allx (560) and the last one (666) are among the 100.                                         -> V = 667
The validation fold is the 500 nodes behind the labelled ones, so allx cannot have fewer than len(y) + 500 rows.
"""
import os
import pickle
from collections import defaultdict

import numpy as np

NUM_ALLX, NUM_LABELLED, NUM_TEST, NUM_FEATURES, NUM_CLASSES = 560, 40, 100, 48, 5
KINDS = {"cora": dict(seed=31, holes=0), "citeseer": dict(seed=32, holes=7)}


def expected_sizes(kind: str):
    """(nodes, features, classes, masked nodes per fold) of the directory write_planetoid_dir(kind) writes."""
    return NUM_ALLX + NUM_TEST + KINDS[kind]["holes"], NUM_FEATURES, NUM_CLASSES, (NUM_LABELLED, 500, NUM_TEST)


def write_planetoid_dir(path: str, kind: str) -> dict:
    import scipy.sparse as sp
    spec = KINDS[kind]
    rng = np.random.default_rng(spec["seed"])
    span = NUM_TEST + spec["holes"]
    num_nodes = NUM_ALLX + span

    def features(rows):
        bag = (rng.random((rows, NUM_FEATURES)) < 0.08).astype(np.float32)
        bag[rng.choice(rows, size=max(2, rows // 40), replace=False)] = 0.0           # documents without any counted word
        return sp.csr_matrix(bag)

    def one_hot(rows):
        table = np.zeros((rows, NUM_CLASSES), dtype=np.int32)
        table[np.arange(rows), rng.integers(0, NUM_CLASSES, size=rows)] = 1
        return table

    allx, ally = features(NUM_ALLX), one_hot(NUM_ALLX)
    tx, ty = features(NUM_TEST), one_hot(NUM_TEST)
    x, y = allx[:NUM_LABELLED], ally[:NUM_LABELLED]
    # the test ids: all of the range behind allx but `holes` of them; its first and last id always present
    inner = NUM_ALLX + 1 + rng.choice(span - 2, size=NUM_TEST - 2, replace=False)
    test_ids = np.concatenate([[NUM_ALLX, NUM_ALLX + span - 1], inner])
    rng.shuffle(test_ids)
    graph = defaultdict(list)
    for node in rng.permutation(num_nodes):
        degree = int(rng.choice([0, 0, 1, 2, 3, 5, 9]))
        neighbours = rng.integers(0, num_nodes, size=degree).tolist()
        if degree >= 3:
            neighbours[-1] = neighbours[0]                                            # a duplicate entry
        graph[int(node)] = [int(n) for n in neighbours]
    for name, obj in (("x", x), ("y", y), ("tx", tx), ("ty", ty), ("allx", allx), ("ally", ally), ("graph", graph)):
        with open(os.path.join(path, "ind.%s.%s" % (kind, name)), "wb") as f:
            pickle.dump(obj, f, protocol=2)
    with open(os.path.join(path, "ind.%s.test.index" % kind), "w") as f:
        f.write("".join("%d\n" % i for i in test_ids))
    return dict(kind=kind, seed=spec["seed"], num_nodes=num_nodes, test_ids=[int(i) for i in test_ids])
