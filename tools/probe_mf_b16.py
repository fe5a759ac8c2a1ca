#!/usr/bin/env python3
"""bf16 multi-frame projection probe: k_mf_forward_b16 / k_mf_backproject_b16 time per batch width and kernel
variant of the launch table (mf_variants("b16", nf): each key with the knob setting that selects it) on a synthetic
bf16 shard (default 65536 x 65536). One JSON line per measurement."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from mpi_cuda_sartsolver_amd.models.rtm import DenseRTM  # noqa: E402
from mpi_cuda_sartsolver_amd.ops import hip  # noqa: E402
from probe import timeit  # noqa: E402


def main():
    k = hip()
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream().cuda_stream
    P, V = (int(v) for v in (sys.argv[1] if len(sys.argv) > 1 else "65536x65536").split("x"))
    m = DenseRTM.synthetic(P, V, 0, seed=1, device=dev, storage="bf16")
    nbytes = m.nbytes
    nfs = [int(v) for v in os.environ.get("PROBE_NF", "16,32,64").split(",")]
    for nf in nfs:
        Xh = torch.rand((nf, m.ld), device=dev).bfloat16()
        Xl = (torch.rand((nf, m.ld), device=dev) * 1e-3).bfloat16()
        Fo = torch.zeros((16, m.nrows_pad, nf), device=dev)
        Wh = torch.rand((nf, m.nrows_pad), device=dev).bfloat16()
        Wl = (torch.rand((nf, m.nrows_pad), device=dev) * 1e-3).bfloat16()
        part = torch.zeros((64, m.ld, nf), device=dev)
        for forward in (True, False) if os.environ.get("PROBE_BWD", "1") == "1" else (True,):
            for var in k.mf_variants("b16", nf, forward):
                env = var.pop("env")
                os.environ.update(env)
                if forward:
                    ns = k.mf_forward_num_splits(m.ld, m.nrows_pad)
                    med, best = timeit(lambda: k.mf_forward_b16(m.A.data_ptr(), m.ld, P, m.nrows_pad, Xh.data_ptr(),
                                                                Xl.data_ptr(), Fo.data_ptr(), ns, s, nf), reps=5)
                else:
                    ns = k.mf_backproject_b16_num_splits(m.ld, P)
                    assert ns <= 64
                    med, best = timeit(lambda: k.mf_backproject_b16(m.A.data_ptr(), m.ld, P, Wh.data_ptr(),
                                                                    Wl.data_ptr(), m.nrows_pad, ns, part.data_ptr(), s,
                                                                    nf), reps=5)
                print(json.dumps(dict(op="mf_forward_b16" if forward else "mf_backproject_b16", nf=nf, nsplit=ns, P=P,
                                      V=V, ms=round(med, 4), GBps=round(nbytes / med / 1e6, 1),
                                      TFLOPs=round(4 * nf * P * V / med / 1e9, 1), env=env, **var)), flush=True)
                for key in env:
                    os.environ.pop(key, None)
        del Xh, Xl, Fo, Wh, Wl, part
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
