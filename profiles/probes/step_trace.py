"""What a step LAUNCHES and what it COMPUTES, as a file two trees can be compared by: for each configuration below the
call runs twice in this process under an armed probe, and the JSON holds the ordered launch list of each run (family, M,
N, K, flags, kernel symbol, grid, block; a second run that repeats the first is stored as "same as run 0") and the
SHA-256 of the bytes of every output (predictions, loss, each parameter gradient, each BatchNorm buffer) that hashes alike
in both runs (see summarise).  Only the package's public surface is used, so the same file runs against any commit:

    python profiles/probes/step_trace.py PARENT.json /other/tree       # another checkout (built), same script
    python profiles/probes/step_trace.py NEW.json . PARENT.json        # this tree; what equals PARENT.json is stored as
                                                                       # "same as baseline", so the file IS the comparison

A host refactor of the step must leave every launch list as it was, and every output whose two runs hash alike (no
free-order atomics in its history) must keep that hash."""
import hashlib
import json
import os
import sys

REPO = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else \
    os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

import torch  # noqa: E402
import mmgnn  # noqa: E402,F401
from mmgnn import model as mm, ops  # noqa: E402
from oracle import fixtures as fx, model as om, train as ot  # noqa: E402

DEV = torch.device("cuda:0")
SEED = 424242
EICU = (1834, 50, 114, 100)
ALL_SITES = ("heads", "conv", "enc2", "enc1")
# (name, graph, hidden, dropout, call, execution switches)
CONFIGS = [
    ("eicu128_train_overlap_off", EICU, 128, 0.2, "train", dict(overlap="off")),
    ("eicu128_train_overlap_on", EICU, 128, 0.2, "train", dict(overlap="on")),
    ("eicu128_train_next_bn_all", EICU, 128, 0.2, "train", dict(next_bn=ALL_SITES)),
    ("eicu128_train_next_bn_none", EICU, 128, 0.2, "train", dict(next_bn=())),
    ("eicu128_train_fused_wgrad_off", EICU, 128, 0.2, "train", dict(fused_wgrad=False)),
    ("eicu128_eval_predict", EICU, 128, 0.2, "predict", {}),
    ("eicu128_eval_impute", EICU, 128, 0.2, "impute", {}),
    ("g500_128_train", (500, 20, 25, 18), 128, 0.2, "train", {}),
    ("g640_256_train_p0", (640, 30, 40, 25), 256, 0.0, "train", {}),
    ("g300_64_train", (300, 12, 15, 10), 64, 0.2, "train", {}),
    ("g300_64_forward", (300, 12, 15, 10), 64, 0.2, "forward", {}),
    ("g300_64_encode", (300, 12, 15, 10), 64, 0.2, "encode", {}),
    ("g400_900labs_128_train_p0", (400, 30, 900, 40), 128, 0.0, "train", {}),
]


def sha(t: torch.Tensor) -> str:
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def run_config(n, hidden, p, call, switches):
    g = fx.graph_from_frames(fx.det_frames(*n))
    gv = om.GraphView(g)
    sd = fx.det_state(gv.num_nodes, hidden)
    cfg = {"model": {"architecture": "RGCN", "hidden_dim": hidden, "num_layers": 2, "dropout": p, "use_batch_norm": True,
                     "activation": "relu"}}
    model = mm.build_model(cfg, (g.node_types, g.edge_types), None).to(DEV)
    gd = g.clone().to(DEV)
    model._init_embeddings(gd)
    model.configure_execution(overlap=switches.get("overlap"), next_bn=switches.get("next_bn"))
    mm.set_fused_wgrad(switches.get("fused_wgrad", True))
    model._dropout_seed = SEED
    ei, ea = g["patient", "has_lab", "lab"].edge_index, g["patient", "has_lab", "lab"].edge_attr
    tr, _, _ = ot.edge_splits(ei.shape[1])
    pi, li, y = ei[0][tr], ei[1][tr], ea[tr].squeeze(-1)
    w = ot.lab_weights(li, y, gv.num_nodes["lab"])
    sup = ot.supervision_mask(int(tr.sum()), 0.2, torch.Generator().manual_seed(1)).to(DEV)
    pid, lid, wsup, ysup = pi.to(DEV), li.to(DEV), w[li].to(DEV)[sup], y.to(DEV)[sup]
    runs = []
    for _ in range(2):
        model.load_state_dict(sd)
        model.zero_grad(set_to_none=True)
        model._pair_cache.clear()                      # both runs build their pair set
        model.train(call not in ("predict", "impute"))
        torch.cuda.synchronize()
        ops.probe_arm(1 << 14)
        outs = {}
        if call == "train":
            pred = model.predict_lab_values(gd, pid, lid)
            loss = ((pred[sup] - ysup).abs() * wsup).mean()
            loss.backward()
            outs.update(pred=pred, loss=loss)
        elif call in ("forward", "encode"):
            res = model(gd) if call == "forward" else model.encode_nodes(gd)
            loss = sum(v.square().sum() for v in res.values())
            loss.backward()
            outs.update({f"out.{t}": v for t, v in res.items()}, loss=loss)
        else:
            with torch.no_grad():
                outs["pred"] = model.predict_lab_values(gd, pid, lid) if call == "predict" else model.impute_lab_matrix(gd)
        torch.cuda.synchronize()
        launches = ops.probe_read()
        grids = ops.probe_grids()
        for k, prm in model.named_parameters():
            if prm.grad is not None:
                outs[f"grad.{k}"] = prm.grad
        for k, b in model.named_buffers():
            outs[f"buf.{k}"] = b
        runs.append({"launches": [[fam, M, N, K, fl, sym, list(gr), bl]
                                  for (_, fam, M, N, K, fl, sym), (gr, bl) in zip(launches, grids)],
                     "sha256": {k: sha(v) for k, v in outs.items()}})
    mm.set_fused_wgrad(True)
    return runs


def summarise(runs):
    """Two runs of one configuration -> its entry of the file: the launch list (of the second run too where it differs),
    and of the outputs that hash alike in both runs ONE SHA-256 over their sorted "name hash" lines when that is all of
    them, else their hashes one by one beside the names of the others (whose hashes say nothing)."""
    r0, r1 = runs
    loose = sorted(k for k in r0["sha256"] if r0["sha256"][k] != r1["sha256"].get(k))
    kept = {k: v for k, v in sorted(r0["sha256"].items()) if k not in loose}
    ent = {"launches": r0["launches"], "launches_run1": "same as run 0" if r1["launches"] == r0["launches"] else r1["launches"],
           "outputs": len(r0["sha256"]), "not_reproducible": loose}
    if loose:
        ent["sha256"] = kept
    else:
        ent["sha256_all_outputs"] = hashlib.sha256("\n".join(f"{k} {v}" for k, v in kept.items()).encode()).hexdigest()
    return ent


def against(ent, base):
    """The entry with everything that equals the baseline's replaced by "same as baseline"; of per-output hashes only
    those the baseline does not have alike, and `changed`: the baseline's reproducible outputs that did not keep their hash."""
    out = {k: ("same as baseline" if base.get(k) == v else v) for k, v in ent.items()}
    if isinstance(out.get("sha256"), dict) and isinstance(base.get("sha256"), dict):
        out["sha256"] = {k: v for k, v in ent["sha256"].items() if base["sha256"].get(k) != v}
        out["changed"] = sorted(k for k, v in base["sha256"].items() if ent["sha256"].get(k) != v)
    return out


def main():
    base = json.load(open(sys.argv[3])) if len(sys.argv) > 3 else None
    out = {}
    for name, n, hidden, p, call, switches in CONFIGS:
        out[name] = summarise(run_config(n, hidden, p, call, switches))
        print(f"{name}: {len(out[name]['launches'])} launches, second run {out[name]['launches_run1']!r:.16}, "
              f"{out[name]['outputs'] - len(out[name]['not_reproducible'])} of {out[name]['outputs']} outputs reproduce",
              flush=True)
        if base is not None:
            out[name] = against(out[name], base[name])
    with open(sys.argv[1], "w") as f:            # one launch / one hash per line: the file diffs line by line
        f.write("{\n")
        for ci, name in enumerate(sorted(out)):
            f.write(f" {json.dumps(name)}: {{\n")
            items = []
            for k, v in out[name].items():
                if k.startswith("launches") and isinstance(v, list):
                    v = "[\n" + ",\n".join("   " + json.dumps(row, separators=(",", ":")) for row in v) + "\n  ]"
                elif isinstance(v, dict):
                    v = "{\n" + ",\n".join(f"   {json.dumps(a)}: {json.dumps(b)}" for a, b in v.items()) + "\n  }"
                else:
                    v = json.dumps(v)
                items.append(f"  {json.dumps(k)}: {v}")
            f.write(",\n".join(items) + "\n }" + (",\n" if ci + 1 < len(out) else "\n"))
        f.write("}\n")


if __name__ == "__main__":
    main()
