"""A seeded writer of a tiny VarMisuse dataset in the reference's raw layout (tasks/varmisuse_task.py:69-136, :265-293):
<dir>/graphs-train, graphs-valid, graphs-test, each holding *.gz files of samples

    {"ContextGraph": {"NodeLabels": {"0": ..., "1": ...}, "Edges": {"Child": [[src, dst], ...], ...}},
     "SymbolCandidates": [{"SymbolDummyNode": id, "IsCorrect": bool}, ...], "SlotDummyNode": id}

tests/golden/make_reference_run_varmisuse.py ran the reference's own loader over exactly these directories; the tests write them
again (same seed, same bytes) and load them with the package's loader.

8 train graphs in two files (one .jsonl.gz, one .json.gz: the two forms read_by_file_suffix decodes), 3 validation and 3 test graphs,
12 .. 40 raw nodes each (the loader adds one node per subtoken).  Covered on purpose:
  * labels longer than 19 characters, upper case, characters outside the alphabet, '{' and '}' (codes 68 and 69);
  * identifiers that split on '_' and camelCase, keyword and punctuation labels that must not be split;
  * an edge type with an empty list ("GuardedBy": []), an edge type absent from the dict ("ReturnsTo"), a "UsesSubtoken" list in
    the file that the loader overwrites;
  * 1, 3, 5 and 7 candidates, the correct one never first in the file when there is a choice;
  * train graph 0 has its slot at node 0 (its padded candidates coincide with the slot), train graph 1 has node 0 as a real
    candidate next to padded ones.
"""
import gzip
import json
import os

import numpy as np

SEED = 41
FOLDS = {"graphs-train": 8, "graphs-valid": 3, "graphs-test": 3}
CANDIDATE_COUNTS = [1, 3, 5, 7]
IDENTIFIERS = ["getValueCount", "HTTPServerName", "my_var_name2", "aVeryLongIdentifierNameThatExceedsNineteen", "index", "i", "tmpBuffer",
               "CONSTANT_VALUE", "node_id", "parseXMLDocument", "x1", "resultList", "_private", "isValid", "ANOTHER_QUITE_LONG_CONSTANT_NAME",
               "naïve", "x→y", "tab\there", "sum$total", "a{b}c"]
KEYWORDS = ["if", "return", "int", "new", "foreach", "void"]
PUNCTUATION = ["{", "}", ";", "(", ")", "=", "==", ".", ",", "[", "]", "+="]
EDGE_TYPES = ["Child", "NextToken", "LastUse", "LastWrite", "LastLexicalUse", "ComputedFrom", "GuardedByNegation", "FormalArgName"]


def _graph(rng, index: int, fold: str) -> dict:
    num_nodes = int(rng.integers(12, 41))
    labels = {}
    for node in range(num_nodes):
        pool = (IDENTIFIERS, KEYWORDS, PUNCTUATION)[int(rng.choice(3, p=[0.6, 0.15, 0.25]))]
        labels[str(node)] = pool[int(rng.integers(0, len(pool)))]
    edges = {}
    for e_type in EDGE_TYPES:
        if e_type == "NextToken":
            pairs = [[i, i + 1] for i in range(num_nodes - 1)]
        else:
            count = int(rng.integers(0, num_nodes))
            pairs = [[int(a), int(b)] for a, b in rng.integers(0, num_nodes, size=(count, 2))]
        if pairs or rng.random() < 0.5:              # (a sparse type is sometimes an empty list, sometimes absent)
            edges[e_type] = pairs
    edges["GuardedBy"] = []
    edges["UsesSubtoken"] = [[0, 1]]                 # overwritten by the loader (:66)
    num_cands = CANDIDATE_COUNTS[index % len(CANDIDATE_COUNTS)]
    first_train = fold == "graphs-train" and index == 0
    second_train = fold == "graphs-train" and index == 1
    slot = 0 if first_train else int(rng.integers(1, num_nodes))
    others = [n for n in range(1 if not second_train else 0, num_nodes) if n != slot]
    picked = [int(n) for n in rng.choice(others, size=num_cands, replace=False)]
    if second_train:
        picked[0] = 0                                # node 0 as a real (wrong) candidate
        picked = list(dict.fromkeys(picked))
        while len(picked) < num_cands:
            picked.append(next(n for n in others if n not in picked))
    correct_at = num_cands - 1 if num_cands > 1 else 0
    candidates = [{"SymbolDummyNode": n, "IsCorrect": i == correct_at} for i, n in enumerate(picked)]
    return {"ContextGraph": {"NodeLabels": labels, "Edges": edges}, "SymbolCandidates": candidates, "SlotDummyNode": slot}


def write_varmisuse_dir(path: str) -> dict:
    """-> {fold: number of graphs}.  The same bytes for the same SEED."""
    rng = np.random.default_rng(SEED)
    for fold, count in FOLDS.items():
        os.makedirs(os.path.join(path, fold), exist_ok=True)
        graphs = [_graph(rng, i, fold) for i in range(count)]
        if fold == "graphs-train":
            with gzip.open(os.path.join(path, fold, "chunk_0000.jsonl.gz"), "wt") as f:
                f.write("".join(json.dumps(g) + "\n" for g in graphs[:5]))
            with gzip.open(os.path.join(path, fold, "chunk_0001.json.gz"), "wt") as f:
                json.dump(graphs[5:], f)
        else:
            with gzip.open(os.path.join(path, fold, "chunk_0000.jsonl.gz"), "wt") as f:
                f.write("".join(json.dumps(g) + "\n" for g in graphs))
    return dict(FOLDS)
