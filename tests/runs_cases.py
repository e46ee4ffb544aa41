"""Helpers of the `--runs` tests (tests/test_runs_host.py, tests/test_gpu_runs.py): per-base bedgraph text <-> run-length bedgraph text.
A run-length record `name s e v` stands for the per-base lines `name p p+1 v`, p = s .. e-1; a record starts a contig iff its name differs
from the previous record's."""
import numpy as np


def parse(text):
    """bedgraph text (per base or run-length) -> [(name, start, end, value)], records being four white-space separated tokens"""
    t = text.split()
    assert len(t) % 4 == 0
    return [(t[i], int(t[i + 1]), int(t[i + 2]), int(t[i + 3])) for i in range(0, len(t), 4)]


def fmt(recs):
    return b"".join(b"%s\t%d\t%d\t%d\n" % r for r in recs)


def to_runs(per_base_text, mode, seed=0):
    """"max": maximal runs; "unit": the file as it is (every per-base file whose contigs start at 0 is a run-length file);
    "cut": maximal runs cut again at seeded random places"""
    if mode == "unit":
        return per_base_text
    recs = parse(per_base_text)
    runs = []
    for name, s, e, v in recs:
        if runs and runs[-1][0] == name and runs[-1][3] == v and runs[-1][2] == s:
            runs[-1][2] = e
        else:
            runs.append([name, s, e, v])
    if mode == "max":
        return fmt(tuple(r) for r in runs)
    assert mode == "cut"
    rng = np.random.default_rng(seed)
    out = []
    for name, s, e, v in runs:
        cuts = []
        if e - s > 1 and rng.random() < 0.5:
            cuts = sorted(set(int(x) for x in rng.integers(s + 1, e, size=int(rng.integers(1, 4)))))
        for a, b in zip([s] + cuts, cuts + [e]):
            out.append((name, a, b, v))
    return fmt(out)


def expand(run_text):
    """the per-base text a run-length text stands for"""
    out = []
    for name, s, e, v in parse(run_text):
        out.append(b"".join(b"%s\t%d\t%d\t%d\n" % (name, p, p + 1, v) for p in range(s, e)))
    return b"".join(out)


def expand_arrays(run_text):
    """-> ([names], [uint16 array per contig], clamped positions): what the run reader must hold for one file"""
    names, arrs, clamped = [], [], 0
    for name, s, e, v in parse(run_text):
        if not names or names[-1] != name:
            names.append(name)
            arrs.append([])
        if v > 65535:
            clamped += e - s
        arrs[-1].append(np.full(e - s, min(v, 65535), dtype=np.uint16))
    return names, [np.concatenate(a) for a in arrs], clamped


def random_pair(rng, w, inc):
    """a random valid pair of run-length files (different run boundaries in the two): 1-6 contigs, lengths at and around multiples of
    inc and w, runs of 1 .. 5000 positions, values 0 .. 70000"""
    n_ctg = int(rng.integers(1, 7))
    lens = []
    for _ in range(n_ctg):
        base = int(rng.choice([inc, w, 2 * w, 3 * inc, w + inc, 5 * w])) * int(rng.integers(1, 4))
        lens.append(max(1, base + int(rng.choice([-1, 0, 1, 7]))))
    texts = []
    for f in range(2):
        recs = []
        for c, n in enumerate(lens):
            p = 0
            while p < n:
                ln = int(rng.choice([1, 1, 2, 17, 300, 5000])) if rng.random() < 0.5 else int(rng.integers(1, 5001))
                e = min(n, p + ln)
                v = int(rng.choice([0, 1, 65535, 65536, 70000])) if rng.random() < 0.15 else int(rng.integers(0, 120))
                recs.append((b"ctg%d" % c, p, e, v))
                p = e
        texts.append(fmt(recs))
    return texts[0], texts[1], lens
