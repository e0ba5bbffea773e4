#!/usr/bin/env python3
"""SHA-256 of everything the three raster calls write, for comparing two builds of the library byte for
byte: run once per build (ICON_AMD_LIB names another libicon_amd.so) and diff the outputs - they must be equal line for line.

  normal maps  every case of render_checker.CASES and normal_grad_oracle.CASES, int32 and int64 faces, rn_lanes 0, 1 and 8:
               images / depth / pix_to_face, and grad_verts for the oracle's seeded grad_field (normal_grad_oracle.grad_field,
               unmasked: every covered pixel enters).  `deferred` is the header's count of faces the sweep handed to the deferred
               list, read out of the forward call's scratch (the backward call defers by the same test on the same boxes)
  silhouette   every case of silhouette_oracle.CASES, int32 and int64 faces: alpha, and grad_verts for the oracle's seeded
               grad_alpha (silhouette_oracle.smooth_field, unmasked)
  scratch      what each *_bytes entry answers for three sets of sizes

    python tools/render_digest.py [--out FILE]
"""
import argparse
import ctypes as C
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = ((6890, 13776, 512, 2), (70316, 140716, 512, 4), (12, 20, 8, 1))      # V, F, S, n_views


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from icon_amd import _lib, _native, render
    import normal_grad_oracle as ngo
    import silhouette_oracle as so

    _lib.require_device()
    dev = torch.device("cuda:0")
    L = _lib.lib()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def sha(t):
        return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()

    def set_lanes(n):
        _lib.check(L.icon_debug_set_option(b"rn_lanes", C.c_int(n)), "rn_lanes")

    both = {1: [], 8: []}                                                 # the cases with a non-empty deferred list under G = 1 / G = 8
    try:
        for name, (fn, S, cams) in ngo.CASES.items():
            v, f = fn()
            g = torch.from_numpy(ngo.grad_field(len(cams), S)).to(dev, torch.float32)
            for dt in (torch.int32, torch.int64):
                ff = torch.from_numpy(f).to(dev, dt)
                for lanes in (0, 1, 8):
                    set_lanes(lanes)
                    vv = torch.from_numpy(v).to(dev).requires_grad_(True)
                    images, depth, pix = render.render_normal_device(vv, ff, cams, S, return_depth=True, return_faces=True, differentiable=True)
                    torch.cuda.synchronize()
                    deferred = int(_native.scratch(dev, 0)[:16].view(torch.int32)[1])      # the header: bad_faces, n_big, n_long, pad
                    images.backward(g)
                    if lanes and deferred and name not in both[lanes]:
                        both[lanes].append(name)
                    say(f"normal {name} {str(dt)[6:]} rn_lanes={lanes} deferred={deferred} images={sha(images)} depth={sha(depth)} "
                        f"pix_to_face={sha(pix)} grad_verts={sha(vv.grad)}")
    finally:
        set_lanes(0)
    say(f"deferred list non-empty under rn_lanes=1: {', '.join(both[1]) or 'NO CASE'}; under rn_lanes=8: {', '.join(both[8]) or 'NO CASE'}")
    for name, (fn, S, cams) in so.CASES.items():
        v, f = fn()
        g = torch.from_numpy(so.smooth_field(len(cams), S)).to(dev, torch.float32)
        for dt in (torch.int32, torch.int64):
            vv = torch.from_numpy(v).to(dev).requires_grad_(True)
            alpha = render.silhouette_device(vv, torch.from_numpy(f).to(dev, dt), cams, S)
            alpha.backward(g)
            say(f"silhouette {name} {str(dt)[6:]} alpha={sha(alpha)} grad_verts={sha(vv.grad)}")
    for V, F, S, n in SIZES:
        out = []
        for entry in ("icon_render_bytes", "icon_silhouette_bytes", "icon_render_normal_backward_bytes"):
            nb = C.c_int64(0)
            _lib.check(getattr(L, entry)(C.c_int64(V), C.c_int64(F), C.c_int(S), C.c_int(n), C.byref(nb)), entry)
            out.append(f"{entry}={nb.value}")
        nb = C.c_int64(0)
        _lib.check(L.icon_query_color_bytes(C.c_int64(V), C.c_int64(F), C.c_int(S), C.byref(nb)), "icon_query_color_bytes")
        say(f"scratch V={V} F={F} S={S} n_views={n}: " + " ".join(out) + f" icon_query_color_bytes={nb.value}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
