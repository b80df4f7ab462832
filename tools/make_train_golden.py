"""Goldens of the reference's own weight-training loop -> tests/golden/train/*.npz.

Runs only where the reference tree exists (oracle/ref_loader.py loads its files by path; nothing of it is copied).  For every
case the reference's ``GCN`` / ``GraphSAGE`` / ``STEGCN`` module (gnn/models/models.py:14-118) in ``train()`` mode runs the
driver's loop (gnn/marglik_training.py:91-93, 159-186) for three epochs over three batches with
``torch.optim.Adam(lr, weight_decay)`` on every parameter whose name has no ``adj``:

    f = model(idx); optimizer.zero_grad(); loss = CrossEntropyLoss()(f, y); loss.backward(); optimizer.step()

Stored (arrays only): the inputs, per parameter its trajectory ``P/<name>`` [steps + 1, ...] (entry 0 = initial, entry s + 1 =
after step s) and its gradients ``G/<name>`` [steps, ...], per hidden layer the keep-masks ``masks_<l>`` [steps, N, H] the
reference's ``nn.Dropout`` drew (a forward hook on ``model.dropout`` compares its input and output; where the input is
exactly zero the draw cannot be seen and does not matter -- stored as kept), the logits ``logits_<s>`` and the loss per step.
A seed is kept only when every parameter's gradient has a non-zero norm at every step.

    python tools/make_train_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
OUT = os.path.join(ROOT, "tests", "golden", "train")

# name -> (kind, kwargs of the case)
CASES = {
    "gcn_plain_p0": ("gcn", dict(p=0.0, symmetric=True)),
    "gcn_plain_p05": ("gcn", dict(p=0.5, symmetric=True)),
    "gcn_resln_p0": ("gcn", dict(p=0.0, res=True, norm="layer", symmetric=True)),
    "gcn_resln_p05": ("gcn", dict(p=0.5, res=True, norm="layer", symmetric=True)),
    "sage_plain_p0": ("sage", dict(p=0.0, symmetric=True)),
    "sage_plain_p05": ("sage", dict(p=0.5, symmetric=True)),
    "sage_resln_p0": ("sage", dict(p=0.0, res=True, norm="layer", symmetric=True)),
    "sage_resln_p05": ("sage", dict(p=0.5, res=True, norm="layer", symmetric=True)),
    "gcn3_resln_p05": ("gcn", dict(p=0.5, res=True, norm="layer", symmetric=True, layers=3)),
    "sage3_plain_p05": ("sage", dict(p=0.5, symmetric=True, layers=3)),
    "sage_tanh_p05": ("sage", dict(p=0.5, symmetric=True, act="tanh")),
    "gcn_tanh_ln_p05": ("gcn", dict(p=0.5, norm="layer", symmetric=True, act="tanh")),
    "gcn_dir_p05": ("gcn", dict(p=0.5, symmetric=False)),
    "sage_dir_resln_p05": ("sage", dict(p=0.5, res=True, norm="layer", symmetric=False)),
    "stegcn_p05": ("stegcn", dict(p=0.5, symmetric=True)),
}


def run_case(ns, torch, kind, seed, p=0.5, res=False, norm=None, symmetric=True, layers=2, act="relu", n=64, f=12, h=8, c=3,
             n_edges=150, n_train=33, batch_size=12, lr=0.01, weight_decay=5e-4, epochs=3):
    from torch.utils.data import DataLoader, TensorDataset

    from make_golden import reference_dense_adj

    g = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, n, (2, n_edges), generator=g)
    X = torch.randn(n, f, generator=g)
    adj0 = reference_dense_adj(torch, ei, n)
    perm = torch.randperm(n, generator=g)
    train_idx = perm[:n_train].clone()
    train_idx[3] = train_idx[5]  # a repeated node id
    train_y = torch.randint(0, c, (n_train,), generator=g)
    loader = DataLoader(TensorDataset(train_idx, train_y), batch_size=batch_size, shuffle=False)
    torch.manual_seed(seed)
    gm = ns.gnn_models
    kw = dict(dropout_p=p, act=act, symmetric=symmetric, norm=norm, res=res)
    if kind == "sage":
        model = gm.GraphSAGE(f, h, c, layers, X, adj0.clone(), None, **kw)
    elif kind == "stegcn":
        model = gm.STEGCN(f, h, c, layers, X, adj0.clone(), threshold=0.5, **kw)
    else:
        model = gm.GCN(f, h, c, layers, X, adj0.clone(), **kw)
    if norm == "layer":  # (LayerNorm starts at weight 1, bias 0: move it so that its gradients are exercised from step 0)
        with torch.no_grad():
            for m in model.norms:
                m.weight.add_(0.2 * torch.randn(h, generator=g))
                m.bias.add_(0.2 * torch.randn(h, generator=g))
    names = [k for k, _ in model.named_parameters() if "adj" not in k]
    params = dict(model.named_parameters())
    optimizer = torch.optim.Adam([params[k] for k in names], lr=lr, weight_decay=weight_decay)  # marglik_training.py:91-93
    criterion = torch.nn.CrossEntropyLoss()
    drawn = []

    def hook(_module, inp, out):
        drawn.append(((out != 0) | (inp[0] == 0)).to(torch.uint8).numpy().copy())

    model.dropout.register_forward_hook(hook)
    traj = {k: [params[k].detach().numpy().copy()] for k in names}
    grads = {k: [] for k in names}
    masks = [[] for _ in range(layers - 1)]
    out = {}
    losses, batch_of_step, ok = [], [], True
    step = 0
    for _ in range(epochs):
        model.train()
        for b, (idx, y) in enumerate(loader):
            drawn.clear()
            fx = model(idx)
            optimizer.zero_grad()
            loss = criterion(fx, y)
            loss.backward()
            optimizer.step()
            assert len(drawn) == layers - 1
            for l in range(layers - 1):
                masks[l].append(drawn[l])
            for k in names:
                gk = params[k].grad.detach().numpy().copy()
                ok = ok and float(np.linalg.norm(gk)) > 0.0
                grads[k].append(gk)
                traj[k].append(params[k].detach().numpy().copy())
            out[f"logits_{step}"] = fx.detach().numpy().copy()
            losses.append(float(loss.detach()))
            batch_of_step.append(b)
            step += 1
    out.update(kind="gcn" if kind == "stegcn" else kind, model=kind, symmetric=symmetric, num_nodes=n, num_layers=layers,
               hidden=h, act=act, res=bool(res), norm="" if norm is None else norm, p=np.float64(p), lr=np.float64(lr),
               weight_decay=np.float64(weight_decay), batch_size=batch_size, epochs=epochs, edge_index=ei.numpy(), X=X.numpy(),
               train_idx=train_idx.numpy(), train_y=train_y.numpy(), names=np.array(names), loss=np.array(losses, dtype=np.float64),
               batch_of_step=np.array(batch_of_step))
    for k in names:
        out["P/" + k] = np.stack(traj[k])
        out["G/" + k] = np.stack(grads[k])
    for l in range(layers - 1):
        out[f"masks_{l}"] = np.stack(masks[l])
    return out, ok


def main():
    import torch

    import ref_loader

    ns = ref_loader.load()
    os.makedirs(OUT, exist_ok=True)
    for name, (kind, kw) in CASES.items():
        for seed in range(200, 240):
            out, ok = run_case(ns, torch, kind, seed, **kw)
            if ok:
                break
        else:
            raise RuntimeError(f"{name}: no seed with non-zero gradients at every step")
        out["seed"] = seed
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **out)
        print(f"{name}: seed {seed}, {os.path.getsize(path) / 1024:.0f} KiB, loss {out['loss'][0]:.4f} -> {out['loss'][-1]:.4f}")


if __name__ == "__main__":
    main()
