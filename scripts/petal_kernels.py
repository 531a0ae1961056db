"""PETAL's own launches alone, for a kernel trace: the magnitude select and the teacher / ranked-restore pass over the bench
U-Net's arena (every trainable tensor a row of the segment table) on `--sets` weight replicas, with a synthetic gradient whose
magnitudes spread over a few binades per tensor, as weight gradients do.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/petal_kernels.py --sets 8

Prints one JSON line: the table's shape, the event-timed average of select and update per call, and the restored share."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from method_bench import MODEL  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quantile", type=float, default=0.03)
    a = ap.parse_args()
    from multimodal_tta_amd import ops
    from multimodal_tta_amd.config import compose
    from multimodal_tta_amd.models import UNet
    from multimodal_tta_amd.registry import get_plugin
    device = torch.device("cuda", 0)
    cfg = compose(overrides=["task=brats", "model=unet", "method=tta_petal"])
    cfg["model"] = dict(MODEL)
    cfg["method"].update(precision="bf16", group=a.sets, lanes=1)
    cfg["method"]["petal"].update(mirror_axes=[], quantile=a.quantile)
    torch.manual_seed(42)
    plug = get_plugin("petal_tta")(cfg).setup(UNet(dict(MODEL)), device)
    ar, table = plug.rt.arena, plug.table
    nt, sets = ar.n_train, min(a.sets, ar.replicas)
    gen = torch.Generator(device=device).manual_seed(1)
    for s in range(sets):
        ar.grads_all[s].copy_(torch.randn(ar.total, generator=gen, device=device) *
                              torch.exp2(torch.randn(ar.total, generator=gen, device=device) * 1.5 - 14.0))
    ar.params_all[:, :nt].add_(1e-3)
    scratch = torch.empty(ops.magnitude_select_scratch(table, sets), dtype=torch.int32, device=device)
    partial = torch.empty(ops.petal_update_partials(nt, sets), dtype=torch.int64, device=device)
    restored = torch.zeros(ar.replicas, dtype=torch.int64, device=device)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    t_sel = t_upd = 0.0
    for rep in range(a.reps + 1):
        ev[0].record()
        ops.magnitude_select_sets(ar.grads_all, table, sets, plug.gamma, scratch)
        ev[1].record()
        ops.petal_update_sets(ar.params_all, plug.teacher, ar.source, ar.grads_all, plug.gamma, table, nt, sets, plug.alpha,
                              partial, restored)
        ev[2].record()
        torch.cuda.synchronize()
        if rep > 0:          # (the first call warms up)
            t_sel += ev[0].elapsed_time(ev[1])
            t_upd += ev[1].elapsed_time(ev[2])
    rows = table.rows
    print(json.dumps({"sets": sets, "rows": len(rows), "rows_chunked": sum(ops.magnitude_select_class(r[1]) for r in rows),
                      "elements": nt, "elements_in_rows": sum(r[1] for r in rows), "select_ms": round(t_sel / a.reps, 4),
                      "update_ms": round(t_upd / a.reps, 4), "restored_share": round(float(restored[0]) / nt, 5)}), flush=True)


if __name__ == "__main__":
    main()
