"""Data-parallel training under `torchrun`: W ranks x A accumulation steps are one process with A W accumulation steps.

Every rank draws all A W micro-batches of an optimizer step (so the CPU mask generator advances identically everywhere), runs those with
index j = rank (mod W), and the gradients of all ranks are summed by ONE collective over one fp32 buffer that `ops.grads_gather` fills in
one launch; `optim.AdamW(..., reducer=GradReducer(...))` then takes its step on that buffer, with grad_scale = 1 / (micro-batches of the
step over all ranks) applied after the sum.  The optimizer state is the same on every rank; `check_in_step` verifies that.

Backends.  nccl (RCCL; one rank per device): `dist.all_reduce` on the device buffer, the host does not wait.  gloo: the buffer goes to a
pinned host mirror, the stream is synchronised, `dist.all_reduce` runs on the CPU tensor, and it comes back - ONE host synchronisation
per optimizer step.  RCCL refuses two ranks on one device and gloo does not, which is what lets a world of 2 - 4 run on a one-GPU box,
for debugging and for this project's tests.  Inference commands keep `sharding.init_from_env`."""
from __future__ import annotations

import os
from typing import Optional, Tuple

import torch
import torch.distributed as dist

BACKENDS = ("nccl", "gloo")
BACKEND_ENV = "PCAD_DDP_BACKEND"
TAIL = 4                    # fp32 elements after the gradients in GradReducer.flat (16 bytes); slot 0 carries the step's partial loss

_OWN_GROUP = False


def backend_from(flag: Optional[str] = None, env=None) -> Optional[str]:
    """the backend a command asks for: its flag, else PCAD_DDP_BACKEND, else None (`init_from_env`'s default)"""
    val = flag or (os.environ if env is None else env).get(BACKEND_ENV) or None
    if val is not None and val not in BACKENDS:
        raise SystemExit(f"the DDP backend must be one of {', '.join(BACKENDS)} (got {val!r})")
    return val


def rank_device(backend: str, local_rank: int, device_count: int) -> str:
    """the device of local rank `local_rank` on a node that shows `device_count` devices: its own with nccl (SystemExit when there is
    none: RCCL needs one device per rank), `local_rank % device_count` with gloo (ranks may share a device)"""
    if backend not in BACKENDS:
        raise SystemExit(f"the DDP backend must be one of {', '.join(BACKENDS)} (got {backend!r})")
    if device_count < 1:
        raise SystemExit("data-parallel training needs a ROCm device; none is visible")
    if backend == "nccl":
        if local_rank >= device_count:
            raise SystemExit(f"LOCAL_RANK {local_rank} has no device of its own ({device_count} visible): RCCL needs one device per rank; "
                             f"start at most {device_count} ranks per node, or pass --ddp_backend gloo to let ranks share a device")
        return f"cuda:{local_rank}"
    return f"cuda:{local_rank % device_count}"


def init_from_env(device: str, backend: Optional[str] = None, device_count: Optional[int] = None) -> Tuple[str, int, int]:
    """-> (device, rank, world).  Plain `python` (no WORLD_SIZE / RANK in the environment): no group, (device, 0, 1).  Under `torchrun`:
    joins the process group on `backend` (nccl when None) and returns this rank's device - `cuda:LOCAL_RANK` with nccl (SystemExit when
    that device does not exist: RCCL needs one device per rank), `cuda:(LOCAL_RANK % device_count)` with gloo (several ranks may share a
    device).  device_count: torch.cuda.device_count() when None."""
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC, before the first GPU call (RCCL needs it here)
    if "WORLD_SIZE" not in os.environ or "RANK" not in os.environ or not dist.is_available():
        return device, 0, 1
    backend = backend or "nccl"
    count = torch.cuda.device_count() if device_count is None else int(device_count)
    device = rank_device(backend, int(os.environ.get("LOCAL_RANK", "0")), count)
    if not dist.is_initialized():
        global _OWN_GROUP
        _OWN_GROUP = True
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.cuda.set_device(torch.device(device))
        if backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=torch.device(device))
        else:
            dist.init_process_group(backend="gloo")
    return device, dist.get_rank(), dist.get_world_size()


def active() -> bool:
    return dist.is_available() and dist.is_initialized()


def barrier():
    if active():
        dist.barrier()


def shutdown():
    """Destroy the process group if `init_from_env` created it (after a barrier), so that no rank sits in a collective afterwards."""
    global _OWN_GROUP
    if _OWN_GROUP and active():
        dist.barrier()
        dist.destroy_process_group()
    _OWN_GROUP = False


def share(batches, rank: int, world: int):
    """rank `rank`'s micro-batches of a step's global list: those with index j = rank (mod world), in order"""
    return [b for j, b in enumerate(batches) if j % world == rank]


def checksum(tensors) -> torch.Tensor:
    """a 64-bit checksum of fp32 tensors as an int64 scalar on their device: the (wrapping) integer sum of their 32-bit patterns"""
    tensors = list(tensors)
    total = torch.zeros((), dtype=torch.int64, device=tensors[0].device)
    for t in tensors:
        total += t.detach().contiguous().view(torch.int32).to(torch.int64).sum()
    return total


def check_in_step(tensors, step: int, what: str = "master weights") -> int:
    """The divergence check: every rank's checksum of `tensors`, all-gathered; a mismatch raises on every rank and names the step.
    -> the checksum.  Synchronises (it is run at checkpoints and at the end)."""
    mine = int(checksum(tensors).item())
    if not active():
        return mine
    world = dist.get_world_size()
    dev = tensors[0].device if dist.get_backend() == "nccl" else torch.device("cpu")
    local = torch.tensor([mine], dtype=torch.int64, device=dev)
    parts = [torch.zeros_like(local) for _ in range(world)]
    dist.all_gather(parts, local)
    sums = [int(p.item()) for p in parts]
    if len(set(sums)) != 1:
        raise RuntimeError(f"the ranks' {what} differ after step {step}: checksums " + ", ".join(f"rank {r}: {s:#018x}" for r, s in enumerate(
            x & 0xFFFFFFFFFFFFFFFF for x in sums)) + " - a backward or a collective that is not reproducible")
    return mine


class GradReducer:
    """The one buffer of a data-parallel step and its collective.  `flat` is fp32 [total + TAIL]: the gradients' slices
    (`ops.grads_flat_plan`), then a tail of TAIL elements whose slot 0 (`loss`) carries the step's partial loss so that the loss needs no
    second collective.  group: a process group (`dist.group.WORLD`), or None - no collective at all, a world of one in-process.
    device: where `flat` lives; a CPU device is taken too (the collective then runs on `flat` itself)."""

    def __init__(self, group, device):
        self.group, self.device = group, torch.device(device)
        self.world = dist.get_world_size(group) if group is not None else 1
        self.backend = dist.get_backend(group) if group is not None else None
        self.total, self.flat, self.host = -1, None, None

    def allocate(self, total: int) -> torch.Tensor:
        """`flat` for `total` gradient elements, zeroed once (the slices' padding stays zero ever after); kept when the size is unchanged"""
        if self.flat is None or self.total != int(total):
            self.total = int(total)
            self.flat = torch.zeros(self.total + TAIL, dtype=torch.float32, device=self.device)
            staged = self.flat.is_cuda and self.backend is not None and self.backend != "nccl"
            self.host = torch.zeros(self.total + TAIL, dtype=torch.float32).pin_memory() if staged else None
        return self.flat

    @property
    def grads(self) -> torch.Tensor:
        return self.flat[:self.total]

    @property
    def loss(self) -> torch.Tensor:
        """slot 0 of the tail, shape [1]: write the rank's sum of loss x scale before the step, read the global loss after it"""
        return self.flat[self.total:self.total + 1]

    def all_reduce(self):
        """`flat` summed over the ranks, in place.  nccl: one collective on the device buffer, no host wait.  gloo with a device buffer:
        device -> pinned host, ONE stream synchronisation, the collective on the CPU tensor, host -> device."""
        if self.group is None:
            return
        if self.host is not None:
            self.host.copy_(self.flat, non_blocking=True)
            torch.cuda.current_stream(self.device).synchronize()
            dist.all_reduce(self.host, group=self.group)
            self.flat.copy_(self.host, non_blocking=True)
        else:
            dist.all_reduce(self.flat, group=self.group)
