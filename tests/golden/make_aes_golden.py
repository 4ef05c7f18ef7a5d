#!/usr/bin/env python3
"""Capture a golden vector for the aesthetic-score head from the reference's own source.

Runs only where a checkout of the reference project is at hand; its root directory is the one argument:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_aes_golden.py REFERENCE_ROOT

evaluations/utils/aes.py imports the OpenAI `clip` package at file scope and cannot be imported here, but its `AE_MLP` class
(lines 48-90) is plain torch: the class is picked out of the parsed module by name and executed as it stands, the way
make_safree_golden.py picks its helpers.  Built with input_size = 64, in eval mode (the Dropouts are the identity), evaluated in
float64.  Only arrays are written (tests/golden/aes_golden.npz): the state dict under the class's own key names -- values rounded
to fp16 first and stored as float16 -- six unit-norm inputs and the six outputs; no reference source text travels.
"""
import ast
import os
import sys

import numpy as np
import torch

SRC = os.path.join("evaluations", "utils", "aes.py")                # under the reference root
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "aes_golden.npz")
INPUT_SIZE = 64


def load_class(src, name="AE_MLP"):
    tree = ast.parse(open(src).read(), src)
    body = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == name]
    assert len(body) == 1, [n.name for n in tree.body if isinstance(n, ast.ClassDef)]
    ns = {"torch": torch, "F": torch.nn.functional}
    exec(compile(ast.Module(body=body, type_ignores=[]), src, "exec"), ns)
    return ns[name]


def main(reference_root):
    torch.manual_seed(20)
    model = load_class(os.path.join(reference_root, SRC))(INPUT_SIZE).eval()
    with torch.no_grad():
        for k, p in model.named_parameters():
            # the default init would give outputs of 1e-2; a wider head with a bias of 5 gives scores of the real head's size
            p.copy_(((2.0 * p) if k.endswith("weight") else p + (5.0 if k == "layers.7.bias" else 0.0)).half().float())
    model = model.double()
    g = torch.Generator().manual_seed(21)
    x = torch.randn(6, INPUT_SIZE, generator=g, dtype=torch.float64)
    x = (x / x.norm(dim=-1, keepdim=True)).float()
    x = x / x.double().norm(dim=-1, keepdim=True).float()             # unit norm to f32 rounding
    with torch.no_grad():
        y = model(x.double())[:, 0]
    store = {f"sd/{k}": v.numpy().astype(np.float16) for k, v in model.state_dict().items()}
    for k, v in model.state_dict().items():
        assert np.array_equal(store[f"sd/{k}"].astype(np.float64), v.numpy()), k
    store["inputs"] = x.numpy()
    store["outputs"] = y.numpy()
    np.savez_compressed(OUT, **store)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes): keys {sorted(model.state_dict())}, outputs {y.tolist()}")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: make_aes_golden.py REFERENCE_ROOT")
    main(sys.argv[1])
