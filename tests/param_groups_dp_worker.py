"""Child process of tests/test_param_groups_gpu.py: the two-group Adam step
under `Trainer(dp=True)` on a world-size-1 RCCL group of its own.
    python tests/param_groups_dp_worker.py OUT.pt [clip_norm]
Two steps of tests/adam_ex_common.run, saved as cpu tensors."""
import os
import socket
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(out, clip):
    from tests.adam_ex_common import run
    from tests.groupsref import pattern_groups
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1,
                            device_id=torch.device("cuda", 0))
    try:
        res = run(2, dp=True, clip_norm=clip, param_groups=pattern_groups())
    finally:
        dist.destroy_process_group()
    torch.save(res, out)


if __name__ == "__main__":
    main(sys.argv[1], float(sys.argv[2]) if len(sys.argv) > 2 else None)
