"""Pairwise comparison of dumped latents.  usage: cmp_latents.py FILE FILE ...
FILE: a torch.save'd list of tensors (element by element: equal, or the largest difference), or a .npy array as
``bench.py --dump-outputs`` writes it (largest difference and relative L2 against the first of the pair)."""
import torch, sys, itertools
import numpy as np


def load(n):
    return [torch.from_numpy(np.load(n))] if n.endswith(".npy") else torch.load(n)


names = sys.argv[1:]
d = {n: load(n) for n in names}
for a, b in itertools.combinations(names, 2):
    res = []
    for x, y in zip(d[a], d[b]):
        if torch.equal(x, y):
            res.append("eq")
            continue
        diff = (x.double() - y.double())
        res.append(f"diff(max {float(diff.abs().max()):.3e}, rel_l2 {float(diff.norm() / x.double().norm().clamp_min(1e-30)):.3e})")
    print("/".join(a.split('/')[-2:]), "/".join(b.split('/')[-2:]), res)
