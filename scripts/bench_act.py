"""The bench U-Net with RELU against the same network with LEAKYRELU, inside ONE process on one GPU: adapted volumes/s of
each activation and the LeakyReLU rate as a fraction of the ReLU rate.

Workload: channels [32, 64, 128, 256, 512], 2 residual units, norm INSTANCE, 4 x 128^3 volumes, S = 10, bf16 precision,
lanes x group volumes in flight (default 3 x 8, what bench.py runs).  Both networks adapt the same seeded volumes,
alternated round by round after a warm-up (graph capture), with at least --volumes timed volumes each.  Prints one JSON line.

usage: python scripts/bench_act.py [--lanes 3] [--group 8] [--volumes 48] [--slope 0.01]
"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")      # one hardware queue per lane (see bench.py)
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multimodal_tta_amd import _lib  # noqa: E402

MODEL = dict(name="unet", in_channels=4, num_classes=3, spatial_dims=3, channels=[32, 64, 128, 256, 512],
             strides=[2, 2, 2, 2], num_res_units=2, norm="INSTANCE", act="RELU", dropout=0.0)


class Network:
    """`lanes` plugins (own model replica, stream and graph each) adapting `group` volumes per launch sequence."""

    def __init__(self, name, act, lanes, group, streams, device, steps):
        from multimodal_tta_amd.config import compose
        from multimodal_tta_amd.models import UNet
        from multimodal_tta_amd.registry import get_plugin

        self.name, self.lanes, self.group = name, lanes, group
        model_cfg = dict(MODEL, act=act)
        cfg = compose(overrides=["task=brats", "model=unet", "method=tta_entmin"])
        cfg["model"] = model_cfg
        cfg["method"].update(steps=steps, precision="bf16", group=group, lanes=lanes)
        self.streams = streams[:lanes]
        self.plugs = []
        for lane in range(lanes):
            torch.manual_seed(42)
            p = get_plugin("entmin_tta")(cfg)
            p.lane = lane
            self.plugs.append(p.setup(UNet(model_cfg), device))

    def round(self, xs):
        for lane in range(self.lanes):
            lo = lane * self.group
            with torch.cuda.stream(self.streams[lane]):
                self.plugs[lane].adapt_volume(xs[lo:lo + self.group])
        return self.lanes * self.group


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=3)
    ap.add_argument("--group", type=int, default=8)
    ap.add_argument("--volumes", type=int, default=48)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--slope", type=float, default=0.01)
    ap.add_argument("--shape", type=int, nargs=3, default=[128, 128, 128])
    a = ap.parse_args()
    from multimodal_tta_amd import ops
    from multimodal_tta_amd.synth import synth_volume
    _lib.load()
    device = torch.device("cuda", 0)
    streams = ops.lane_streams(a.lanes, device)
    n_in = a.lanes * a.group
    xs = torch.stack([synth_volume(i, 4, tuple(a.shape), 3)["image"] for i in range(n_in)]).to(device)
    nets = [Network("relu", "RELU", a.lanes, a.group, streams, device, a.steps),
            Network("leaky_relu", ("LEAKYRELU", {"negative_slope": a.slope}), a.lanes, a.group, streams, device, a.steps)]
    for net in nets:                                    # warm-up: capture
        net.round(xs)
    torch.cuda.synchronize()
    t = {net.name: 0.0 for net in nets}
    n = {net.name: 0 for net in nets}
    while min(n.values()) < a.volumes:                  # alternated, one round per network and turn
        for net in nets:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n[net.name] += net.round(xs)
            torch.cuda.synchronize()
            t[net.name] += time.perf_counter() - t0
    rate = {k: round(n[k] / t[k], 2) for k in n}
    print(json.dumps({"workload": f"unet INSTANCE {a.shape[0]}x{a.shape[1]}x{a.shape[2]} S={a.steps} bf16",
                      "lanes": a.lanes, "group": a.group, "negative_slope": a.slope, "timed_volumes": n,
                      "relu_volumes_per_s": rate["relu"], "leaky_relu_volumes_per_s": rate["leaky_relu"],
                      "leaky_over_relu": round(rate["leaky_relu"] / rate["relu"], 3),
                      "peak_memory_gb": round(torch.cuda.max_memory_allocated(device) / 2 ** 30, 2)}), flush=True)


if __name__ == "__main__":
    main()
