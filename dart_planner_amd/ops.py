"""Array front-end of the C ABI: shapes, allocation and pointer hand-over.

``Ops`` is written against a tiny array-backend protocol so that the *same* host logic serves
PyTorch-ROCm tensors in production (:class:`TorchBackend`: CUDA tensors only, current HIP
stream, libse3mpc.so) and plain host buffers in the CPU test-suite (``tests/emu``).  PyTorch is
plumbing here -- device memory and streams -- every number is produced by the HIP kernels.

Layouts (include/se3mpc.h): evaluation ops use the lane layout ``[row][b]`` (one trajectory per
lane), the solver uses the problem layout ``[b][row]`` (the reference's decision-vector packing,
src/dart_planner/planning/se3_mpc_planner.py:361-376).
"""
from __future__ import annotations

from typing import Optional, Tuple

import ctypes as _C

import numpy as np

from .capi import (CONTROLLER_STATE_WORDS, LATENCY_MAX_DEPTH, LATENCY_STATE_WORDS, MISSION_STATE_WORDS, MIXER_STATE_WORDS, ONBOARD_STATE_WORDS,
                   SMOOTHER_STATE_WORDS, SE3MPC_MAX_SPHERES, SE3MPC_MAX_TRACKS, ControllerParams, Library, MissionParams, MixerParams, OnboardParams, Params,
                   SimulatorParams, SmootherParams, SolveInfo, UFieldDesc, get_library)

INFO_DTYPE = np.dtype([("fun", "<f8"), ("nit", "<i4"), ("nfev", "<i4"), ("status", "<i4"), ("task", "<i4")])
assert INFO_DTYPE.itemsize == 24


class TorchBackend:
    """PyTorch-ROCm tensors on a HIP device.  Refuses CPU tensors: there is no CPU path."""
    graph_capable = True          # launches go to torch's current stream: a torch.cuda.graph capture records them

    def __init__(self, device=None):
        import torch
        self.torch = torch
        if not torch.cuda.is_available():
            raise RuntimeError("dart_planner_amd needs a HIP device (torch.cuda.is_available() is False); "
                               "there is no CPU fallback")
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        self._dt = {"f32": torch.float32, "f64": torch.float64, "i32": torch.int32, "i64": torch.int64,
                    "u8": torch.uint8}

    def empty(self, shape, kind):
        return self.torch.empty(shape, dtype=self._dt[kind], device=self.device)

    def suffix(self, a) -> str:
        if a.dtype == self.torch.float32:
            return "f32"
        if a.dtype == self.torch.float64:
            return "f64"
        raise TypeError(f"se3mpc kernels compute in float32 or float64, got {a.dtype}")

    def check(self, a, name: str):
        if not self.torch.is_tensor(a) or not a.is_cuda:
            raise TypeError(f"{name}: expected a CUDA (HIP) tensor; there is no CPU path")
        if a.device != self.device:
            raise ValueError(f"{name}: tensor on {a.device}, backend on {self.device}")
        if not a.is_contiguous():
            raise ValueError(f"{name}: tensor must be contiguous")
        return a

    def ptr(self, a) -> int:
        return 0 if a is None else a.data_ptr()

    def is_host_mapped(self, a) -> bool:
        return self.torch.is_tensor(a) and not a.is_cuda and a.is_pinned() and a.is_contiguous()

    def stream(self) -> int:
        return self.torch.cuda.current_stream(self.device).cuda_stream

    def to_host(self, a) -> np.ndarray:
        return a.detach().cpu().numpy()

    def from_host(self, a: np.ndarray):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.device)

    def elements_from(self, a) -> int:
        """How many elements of a's dtype lie between a's first element and the end of its storage (views into a larger tensor reach
        past their own numel): what a kernel that strides from a.data_ptr() may legally touch."""
        return (a.untyped_storage().nbytes() - a.storage_offset() * a.element_size()) // a.element_size()


class Ops:
    """Shape-checked calls into libse3mpc for one array backend."""

    def __init__(self, backend=None, library: Optional[Library] = None):
        self.lib = library if library is not None else get_library()
        self.be = backend if backend is not None else TorchBackend()

    # ------------------------------------------------------------------ helpers
    def _lane(self, a, rows: int, name: str):
        self.be.check(a, name)
        if a.ndim != 2 or a.shape[0] != rows:
            raise ValueError(f"{name}: expected shape ({rows}, ld), got {tuple(a.shape)}")
        return a

    def _same(self, ref, *others):
        suf = self.be.suffix(ref)
        for o in others:
            if o is not None and (self.be.suffix(o) != suf or o.shape[-1] != ref.shape[-1]):
                raise ValueError("all lane-layout operands must share dtype and leading dimension")
        return suf

    def _spheres(self, spheres, suf) -> int:
        """A sphere table (K <= SE3MPC_MAX_SPHERES, 4) rows (cx, cy, cz, r) of the call's dtype -> K."""
        self.be.check(spheres, "spheres")
        if spheres.ndim != 2 or spheres.shape[1] != 4 or spheres.shape[0] > SE3MPC_MAX_SPHERES or self.be.suffix(spheres) != suf:
            raise ValueError(f"spheres: expected (K<={SE3MPC_MAX_SPHERES}, 4) {suf}, got {tuple(spheres.shape)}")
        return spheres.shape[0]

    def _sphere_vel(self, sphere_vel, sphere_t0, K: int, suf) -> tuple:
        """The velocity table (K, 3) rows (vx, vy, vz) beside a sphere table of K rows -> the two arguments the moving entries take
        after ``spheres``."""
        self.be.check(sphere_vel, "sphere_vel")
        if sphere_vel.ndim != 2 or tuple(sphere_vel.shape) != (K, 3) or self.be.suffix(sphere_vel) != suf:
            raise ValueError(f"sphere_vel: expected ({K}, 3) {suf} beside the sphere table, got {tuple(sphere_vel.shape)}")
        return (self.be.ptr(sphere_vel if K else None), float(sphere_t0))

    def _tracks(self, tracks, lead: tuple, N: int, K: int, suf) -> int:
        """A slab of tracked spheres ``lead`` + (N, Kt, 4) rows (x, y, z, r) of the call's dtype beside a moving table of K rows -> Kt."""
        self.be.check(tracks, "tracks")
        nl = len(lead)
        if (tracks.ndim != nl + 3 or tuple(tracks.shape[:nl]) != tuple(lead) or tracks.shape[nl] != N or tracks.shape[nl + 2] != 4
                or tracks.shape[nl + 1] > SE3MPC_MAX_TRACKS or K + tracks.shape[nl + 1] > SE3MPC_MAX_SPHERES or self.be.suffix(tracks) != suf):
            raise ValueError(f"tracks: expected {tuple(lead) + (N,)} + (Kt<={SE3MPC_MAX_TRACKS}, 4) {suf} with K + Kt <= {SE3MPC_MAX_SPHERES}, "
                             f"got {tuple(tracks.shape)}")
        return tracks.shape[nl + 1]

    @staticmethod
    def _B(ld: int, B: Optional[int]) -> int:
        B = ld if B is None else int(B)
        if B < 0 or B > ld:
            raise ValueError(f"B={B} outside [0, ld={ld}]")
        return B

    # ------------------------------------------------------------------ lane layout
    def init(self, params: Params, p0, v0, goal, project: bool = False, B: Optional[int] = None):
        """a3 (+a4 projection): -> X0 (9N, ld)."""
        N = params.horizon
        self._lane(p0, 3, "p0"); self._lane(v0, 3, "v0")
        if params.has_goal:
            self._lane(goal, 3, "goal")
        suf = self._same(p0, v0, goal if params.has_goal else None)
        ld = p0.shape[1]
        X0 = self.be.empty((9 * N, ld), suf)
        self.lib.call("init", suf, self._B(ld, B), ld, self.be.ptr(p0), self.be.ptr(v0),
                      self.be.ptr(goal if params.has_goal else None), int(bool(project)), self.be.ptr(X0),
                      self.be.stream(), params=params)
        return X0

    def cost_grad(self, params: Params, X, goal, want_grad: bool = True, B: Optional[int] = None):
        """a5 + a6: -> (f (ld,), g (9N, ld) | None)."""
        N = params.horizon
        self._lane(X, 9 * N, "X")
        if params.has_goal:
            self._lane(goal, 3, "goal")
        suf = self._same(X, goal if params.has_goal else None)
        ld = X.shape[1]
        f = self.be.empty((ld,), suf)
        g = self.be.empty((9 * N, ld), suf) if want_grad else None
        self.lib.call("cost_grad", suf, self._B(ld, B), ld, self.be.ptr(X),
                      self.be.ptr(goal if params.has_goal else None), self.be.ptr(f), self.be.ptr(g),
                      self.be.stream(), params=params)
        return f, g

    def dynamics_residual(self, params: Params, X, p0, v0, B: Optional[int] = None):
        """a8: -> R (6N, ld)."""
        N = params.horizon
        self._lane(X, 9 * N, "X"); self._lane(p0, 3, "p0"); self._lane(v0, 3, "v0")
        suf = self._same(X, p0, v0)
        ld = X.shape[1]
        R = self.be.empty((6 * N, ld), suf)
        self.lib.call("dynamics_residual", suf, self._B(ld, B), ld, self.be.ptr(X), self.be.ptr(p0), self.be.ptr(v0),
                      self.be.ptr(R), self.be.stream(), params=params)
        return R

    def obstacle_residual(self, params: Params, X, spheres, materialize: bool = True, reduce: bool = True,
                          B: Optional[int] = None):
        """a9: spheres (K, 4) = (cx, cy, cz, r) -> (C (N*K, ld) | None, cmin (ld,) | None, viol (ld,) | None)."""
        N = params.horizon
        self._lane(X, 9 * N, "X")
        self.be.check(spheres, "spheres")
        if spheres.ndim != 2 or spheres.shape[1] != 4 or spheres.shape[0] > SE3MPC_MAX_SPHERES:
            raise ValueError(f"spheres: expected (K<={SE3MPC_MAX_SPHERES}, 4), got {tuple(spheres.shape)}")
        suf = self.be.suffix(X)
        if self.be.suffix(spheres) != suf:
            raise ValueError("spheres dtype must match X")
        K, ld = spheres.shape[0], X.shape[1]
        Cm = self.be.empty((N * K, ld), suf) if materialize else None
        cmin = self.be.empty((ld,), suf) if reduce else None
        viol = self.be.empty((ld,), suf) if reduce else None
        self.lib.call("obstacle_residual", suf, self._B(ld, B), ld, self.be.ptr(X), self.be.ptr(spheres), K,
                      self.be.ptr(Cm), self.be.ptr(cmin), self.be.ptr(viol), self.be.stream(), params=params)
        return Cm, cmin, viol

    def physical_constraints(self, params: Params, X, B: Optional[int] = None):
        """a10: -> C (4N, ld)."""
        N = params.horizon
        self._lane(X, 9 * N, "X")
        suf, ld = self.be.suffix(X), X.shape[1]
        Cm = self.be.empty((4 * N, ld), suf)
        self.lib.call("physical_constraints", suf, self._B(ld, B), ld, self.be.ptr(X), self.be.ptr(Cm),
                      self.be.stream(), params=params)
        return Cm

    def extract(self, params: Params, T, B: Optional[int] = None):
        """a11 + a12 on the T block (3N, ld): -> acc, att, rates (3N, ld), thrust (N, ld)."""
        N = params.horizon
        self._lane(T, 3 * N, "T")
        suf, ld = self.be.suffix(T), T.shape[1]
        acc, att, rates = (self.be.empty((3 * N, ld), suf) for _ in range(3))
        thrust = self.be.empty((N, ld), suf)
        self.lib.call("extract", suf, self._B(ld, B), ld, self.be.ptr(T), self.be.ptr(acc), self.be.ptr(att),
                      self.be.ptr(rates), self.be.ptr(thrust), self.be.stream(), params=params)
        return acc, att, rates, thrust

    def rollout_cost_grad(self, params: Params, p0, v0, goal, T, want_grad: bool = True, want_states: bool = False,
                          B: Optional[int] = None, out=None, key=None, index_base: int = 0, wave_keys=None):
        """Shooting-form rollout + cost (+ gradient wrt T, + rolled-out states).
        -> (cost (ld,), gradT (3N, ld) | None, P (3N, ld) | None, V (3N, ld) | None).
        ``out=(cost, gradT)`` reuses preallocated outputs (the benchmark's steady state).
        ``key`` (int64 (1,)) receives the fused batch argmin: min over b of (orderable cost bits << 32 |
        index_base + b) -- the kernel writes one partial key per wavefront (``wave_keys``, int64
        (ceil(ld/64),), allocated here unless given) and se3mpc_reduce_keys folds them.  Pass
        ``wave_keys`` alone to defer the fold (bucketed use, see bench.py)."""
        N = params.horizon
        self._lane(p0, 3, "p0"); self._lane(v0, 3, "v0"); self._lane(T, 3 * N, "T")
        if params.has_goal:
            self._lane(goal, 3, "goal")
        suf = self._same(T, p0, v0, goal if params.has_goal else None)
        ld = T.shape[1]
        if out is not None:
            cost, gradT = out
        else:
            cost = self.be.empty((ld,), suf)
            gradT = self.be.empty((3 * N, ld), suf) if want_grad else None
        P = self.be.empty((3 * N, ld), suf) if want_states else None
        V = self.be.empty((3 * N, ld), suf) if want_states else None
        nB = self._B(ld, B)
        if key is not None and wave_keys is None:
            wave_keys = self.be.empty(((nB + 63) // 64,), "i64")
        self.lib.call("rollout_cost_grad", suf, nB, ld, self.be.ptr(p0), self.be.ptr(v0),
                      self.be.ptr(goal if params.has_goal else None), self.be.ptr(T), self.be.ptr(cost),
                      self.be.ptr(gradT), self.be.ptr(P), self.be.ptr(V), self.be.ptr(wave_keys), int(index_base),
                      self.be.stream(), params=params)
        if key is not None and nB > 0:
            self.lib.reduce_keys(self.be.ptr(wave_keys), (nB + 63) // 64, 1, self.be.ptr(key), self.be.stream())
        return cost, gradT, P, V

    def reduce_keys(self, wave_keys, keys_out):
        """wave_keys int64 (nbatch, per_batch) -> keys_out int64 (nbatch,)."""
        nb, per = wave_keys.shape
        self.lib.reduce_keys(self.be.ptr(wave_keys), per, nb, self.be.ptr(keys_out), self.be.stream())
        return keys_out

    def shooting_finish(self, params: Params, T, wave_keys, state, out, key_out=None, spheres=None, obstacle_weight: float = 0.0, B: Optional[int] = None,
                        index_base: int = 0):
        """The tail of a shooting-form plan in one launch (``se3mpc_shooting_finish_*``): fold `wave_keys` (int64, flat), roll the winning column of
        T (3N, ld) out from state = float64 (9,) [p0 | v0 | goal], extract, and write float64 out (19 N + 3,) = [P | V | T | acc | att | rates | thrust |
        cost | penalty | cost + penalty]; key_out: int64 (1,) or None.  state, out and key_out may be pinned host tensors (read / written in place
        over the host link); spheres: float64 (K, 4) device tensor or None."""
        N = params.horizon
        self._lane(T, 3 * N, "T")
        suf = self.be.suffix(T)
        for nm, a, n in (("state", state, 9), ("out", out, 19 * N + 3), ("key_out", key_out, 1)):
            if a is None and nm == "key_out":
                continue
            if not (self.be.is_host_mapped(a) or (self.be.check(a, nm) is a)):
                raise TypeError(f"{nm}: expected a device tensor or a pinned host tensor")
            if int(np.prod(a.shape)) < n or str(a.dtype).rsplit(".", 1)[-1] != ("int64" if nm == "key_out" else "float64"):
                raise ValueError(f"{nm}: expected at least {n} {'int64' if nm == 'key_out' else 'float64'} values")
        K = 0
        if spheres is not None:
            self.be.check(spheres, "spheres")
            if spheres.ndim != 2 or spheres.shape[1] != 4 or spheres.shape[0] > SE3MPC_MAX_SPHERES or str(spheres.dtype).rsplit(".", 1)[-1] != "float64":
                raise ValueError(f"spheres: expected float64 (K<={SE3MPC_MAX_SPHERES}, 4), got {tuple(spheres.shape)} {spheres.dtype}")
            K = spheres.shape[0]
        self.be.check(wave_keys, "wave_keys")
        ld = T.shape[1]
        self.lib.call("shooting_finish", suf, self._B(ld, B), ld, self.be.ptr(T), self.be.ptr(wave_keys), int(np.prod(wave_keys.shape)), int(index_base),
                      self.be.ptr(state), self.be.ptr(spheres if K else None), K, float(obstacle_weight), self.be.ptr(out), self.be.ptr(key_out),
                      self.be.stream(), params=params)
        return out

    def rollout_cost_grad_batched(self, params: Params, p0, v0, goal, T, cost, gradT, wave_keys=None, index_base: int = 0):
        """`nbatch` independent batches in one launch.  p0, v0, goal: (nbatch, 3, ld); T, gradT:
        (nbatch, 3N, ld); cost: (nbatch, ld); wave_keys: int64 (nbatch, ceil(ld/64)) or None (fold with
        :meth:`reduce_keys`).  Outputs are caller-allocated (steady-state use)."""
        N = params.horizon
        nb, _, ld = T.shape
        for a, shp, nm in ((p0, (nb, 3, ld), "p0"), (v0, (nb, 3, ld), "v0"), (T, (nb, 3 * N, ld), "T"),
                           (cost, (nb, ld), "cost"), (gradT, (nb, 3 * N, ld), "gradT")):
            self.be.check(a, nm)
            if tuple(a.shape) != shp:
                raise ValueError(f"{nm}: expected {shp}, got {tuple(a.shape)}")
        if params.has_goal:
            self.be.check(goal, "goal")
        suf = self.be.suffix(T)
        self.lib.call("rollout_cost_grad_batched", suf, ld, ld, nb, self.be.ptr(p0), self.be.ptr(v0),
                      self.be.ptr(goal if params.has_goal else None), self.be.ptr(T), self.be.ptr(cost),
                      self.be.ptr(gradT), self.be.ptr(wave_keys), int(index_base), self.be.stream(), params=params)
        return cost, gradT

    def rollout_obstacles(self, params: Params, p0, v0, goal, T, spheres, want_grad: bool = True, B: Optional[int] = None,
                          wave_keys=None, index_base: int = 0, out=None):
        """Rollout + cost (+ gradient) fused with the sphere-obstacle residuals of the rolled-out positions.
        -> (cost (ld,), gradT (3N, ld) | None, cmin (ld,), viol (ld,)).  ``out=(cost, gradT, cmin, viol)`` reuses
        preallocated outputs."""
        N = params.horizon
        self._lane(p0, 3, "p0"); self._lane(v0, 3, "v0"); self._lane(T, 3 * N, "T")
        if params.has_goal:
            self._lane(goal, 3, "goal")
        suf = self._same(T, p0, v0, goal if params.has_goal else None)
        self._spheres(spheres, suf)
        ld = T.shape[1]
        if out is not None:
            cost, gradT, cmin, viol = out
        else:
            cost = self.be.empty((ld,), suf)
            gradT = self.be.empty((3 * N, ld), suf) if want_grad else None
            cmin, viol = self.be.empty((ld,), suf), self.be.empty((ld,), suf)
        self.lib.call("rollout_obstacles", suf, self._B(ld, B), ld, self.be.ptr(p0), self.be.ptr(v0),
                      self.be.ptr(goal if params.has_goal else None), self.be.ptr(T), self.be.ptr(cost), self.be.ptr(gradT),
                      self.be.ptr(spheres), spheres.shape[0], self.be.ptr(cmin), self.be.ptr(viol), self.be.ptr(wave_keys),
                      int(index_base), self.be.stream(), params=params)
        return cost, gradT, cmin, viol

    def rollout_obstacles_batched(self, params: Params, p0, v0, goal, T, spheres, cost, gradT, cmin, viol, wave_keys=None,
                                  index_base: int = 0):
        """`nbatch` independent batches of the fused rollout + obstacle kernel in one launch (one shared sphere table).
        p0, v0, goal: (nbatch, 3, ld); T, gradT: (nbatch, 3N, ld); cost, cmin, viol: (nbatch, ld); caller-allocated."""
        N = params.horizon
        nb, _, ld = T.shape
        for a, shp, nm in ((p0, (nb, 3, ld), "p0"), (v0, (nb, 3, ld), "v0"), (T, (nb, 3 * N, ld), "T"), (cost, (nb, ld), "cost"),
                           (gradT, (nb, 3 * N, ld), "gradT"), (cmin, (nb, ld), "cmin"), (viol, (nb, ld), "viol")):
            if a is None and nm in ("gradT", "cmin", "viol"):
                continue
            self.be.check(a, nm)
            if tuple(a.shape) != shp:
                raise ValueError(f"{nm}: expected {shp}, got {tuple(a.shape)}")
        if params.has_goal:
            self.be.check(goal, "goal")
        suf = self.be.suffix(T)
        self._spheres(spheres, suf)
        self.lib.call("rollout_obstacles_batched", suf, ld, ld, nb, self.be.ptr(p0), self.be.ptr(v0),
                      self.be.ptr(goal if params.has_goal else None), self.be.ptr(T), self.be.ptr(cost), self.be.ptr(gradT),
                      self.be.ptr(spheres), spheres.shape[0], self.be.ptr(cmin), self.be.ptr(viol), self.be.ptr(wave_keys),
                      int(index_base), self.be.stream(), params=params)
        return cost, gradT, cmin, viol

    def rollout_iterate(self, params: Params, p0, v0, goal, T, iters: int, step: float, T_out=None, want_grad: bool = True,
                        want_first_cost: bool = False, B: Optional[int] = None, out=None, wave_keys=None, index_base: int = 0,
                        spheres=None, obstacle_weight: float = 1000.0, want_penalty: bool = True):
        """`iters` projected-gradient iterations of the shooting form in ONE launch (thrust sequences stay in registers), then one
        last evaluation.  Single batch: p0, v0, goal (3, ld), T (3N, ld); multi-batch (grid.y): leading batch axis on every operand.
        -> dict(T (like T), cost, gradT | None, cost_first | None).  ``out=(T_out, cost, gradT)`` reuses preallocated outputs;
        T_out may be T itself (in place).
        spheres (K, 4) rows (cx, cy, cz, r): the obstacle-aware loop (se3mpc_rollout_iterate_obstacles_*: the build's extension) --
        the objective gains obstacle_weight * sum max(0, -(|P_k - c_j|^2 - (r_j + safety_margin)^2))^2 and the dict a ``penalty`` entry."""
        N = params.horizon
        batched = T.ndim == 3
        nb = T.shape[0] if batched else 1
        ld = T.shape[-1]
        lead = (nb,) if batched else ()
        for a, rows, nm in ((p0, 3, "p0"), (v0, 3, "v0"), (T, 3 * N, "T")) + (((goal, 3, "goal"),) if params.has_goal else ()):
            self.be.check(a, nm)
            if tuple(a.shape) != lead + (rows, ld):
                raise ValueError(f"{nm}: expected {lead + (rows, ld)}, got {tuple(a.shape)}")
        suf = self.be.suffix(T)
        if out is not None:
            T_out, cost, gradT = out
        else:
            T_out = T_out if T_out is not None else self.be.empty(lead + (3 * N, ld), suf)
            cost = self.be.empty(lead + (ld,), suf)
            gradT = self.be.empty(lead + (3 * N, ld), suf) if want_grad else None
        cost_first = self.be.empty(lead + (ld,), suf) if want_first_cost else None
        nB = self._B(ld, B)
        if spheres is not None:
            self._spheres(spheres, suf)
            penalty = self.be.empty(lead + (ld,), suf) if want_penalty else None
            self.lib.call("rollout_iterate_obstacles", suf, nB, ld, nb, int(iters), float(step), self.be.ptr(p0), self.be.ptr(v0),
                          self.be.ptr(goal if params.has_goal else None), self.be.ptr(T), self.be.ptr(T_out), self.be.ptr(cost_first),
                          self.be.ptr(cost), self.be.ptr(gradT), self.be.ptr(spheres if spheres.shape[0] else None), spheres.shape[0],
                          float(obstacle_weight), self.be.ptr(penalty), self.be.ptr(wave_keys), int(index_base), self.be.stream(),
                          params=params)
            return dict(T=T_out, cost=cost, gradT=gradT, cost_first=cost_first, penalty=penalty)
        self.lib.call("rollout_iterate", suf, nB, ld, nb, int(iters), float(step), self.be.ptr(p0), self.be.ptr(v0),
                      self.be.ptr(goal if params.has_goal else None), self.be.ptr(T), self.be.ptr(T_out), self.be.ptr(cost_first),
                      self.be.ptr(cost), self.be.ptr(gradT), self.be.ptr(wave_keys), int(index_base), self.be.stream(), params=params)
        return dict(T=T_out, cost=cost, gradT=gradT, cost_first=cost_first)

    def projected_step(self, params: Params, T, gradT, step: float, out=None, B: Optional[int] = None):
        """One descent step as its own launch: clip(T - step * gradT, thrust box) -> (3N, ld)."""
        N = params.horizon
        self._lane(T, 3 * N, "T"); self._lane(gradT, 3 * N, "gradT")
        suf = self._same(T, gradT)
        ld = T.shape[1]
        T_out = out if out is not None else self.be.empty((3 * N, ld), suf)
        self.lib.call("projected_step", suf, self._B(ld, B), ld, float(step), self.be.ptr(T), self.be.ptr(gradT), self.be.ptr(T_out),
                      self.be.stream(), params=params)
        return T_out

    def is_plan_valid(self, params: Params, P, V=None, B: Optional[int] = None):
        """a16: -> int32 (ld,)."""
        N = params.horizon
        self._lane(P, 3 * N, "P")
        if V is not None:
            self._lane(V, 3 * N, "V")
        suf = self._same(P, V)
        ld = P.shape[1]
        valid = self.be.empty((ld,), "i32")
        self.lib.call("is_plan_valid", suf, self._B(ld, B), ld, self.be.ptr(P), self.be.ptr(V), self.be.ptr(valid),
                      self.be.stream(), params=params)
        return valid

    def argmin(self, cost, index_base: int = 0, out=None):
        """-> int64 (1,) holding the packed unsigned key (cost bits << 32 | index)."""
        self.be.check(cost, "cost")
        suf = self.be.suffix(cost)
        key = out if out is not None else self.be.empty((1,), "i64")
        self.lib.call("argmin", suf, int(cost.shape[0]), self.be.ptr(cost), int(index_base), self.be.ptr(key),
                      self.be.stream())
        return key

    def decode_key(self, key) -> Tuple[int, float]:
        k = int(self.be.to_host(key).reshape(-1)[0]) & 0xFFFFFFFFFFFFFFFF
        return self.lib.key_index(k), self.lib.key_cost(k)

    def population_sums(self, X, cost=None, temperature: float = 1.0, cost_ref: float = 0.0, ref_key=None, B: Optional[int] = None):
        """out[r] = sum_b w_b X[r][b] (r < rows), out[rows] = sum_b w_b in float64; w = 1, or the MPPI weight
        exp(-(cost - cost_ref) / temperature) with cost_ref taken from the packed argmin key `ref_key` (device) when
        given.  X: (rows, ld) lane layout.  -> device float64 (rows + 1,)."""
        self.be.check(X, "X")
        if X.ndim != 2:
            raise ValueError("X: expected (rows, ld)")
        rows, ld = X.shape
        B = self._B(ld, B)
        suf = self.be.suffix(X)
        if cost is not None and (self.be.suffix(self.be.check(cost, "cost")) != suf or cost.shape[-1] < B):
            raise ValueError("cost: same dtype as X and at least B entries")
        out = self.be.empty((rows + 1,), "f64")
        work = self.be.empty((self.lib.population_workspace(rows, B),), "f64")
        self.lib.call("population_sums", suf, rows, B, ld, self.be.ptr(X), self.be.ptr(cost), float(cost_ref), self.be.ptr(ref_key),
                      float(temperature), self.be.ptr(out), self.be.ptr(work), self.be.stream())
        return out

    def _mppi_operands(self, params: Params, U, p0=None, v0=None, goal=None):
        N = params.horizon
        self._lane(U, 3 * N, "U")
        if p0 is not None:
            self._lane(p0, 3, "p0"); self._lane(v0, 3, "v0")
            if params.has_goal:
                self._lane(goal, 3, "goal")
        return self._same(U, p0, v0, goal if params.has_goal else None), U.shape[1]

    def _mppi_call(self, base, tail, params, p0, v0, goal, U, n_samples, iters, sigma, temperature, seed, iter_base, index_base, spheres,
                   obstacle_weight, U_out, want_trace, want_keys, iter_offset, B, out, sphere_vel=None, sphere_t0=0.0, tracks=None):
        """The operand checks, output allocation and call shared by :meth:`mppi` and :meth:`mppi_split`; ``tail``: the arguments between
        ``keys`` and ``stream``; ``sphere_vel``: the moving entry's two arguments go in after ``spheres``; ``tracks``: (N, Kt, 4) or
        (ld, N, Kt, 4), the tracks entry's three arguments go in after ``K``."""
        suf, ld = self._mppi_operands(params, U, p0, v0, goal)
        N = params.horizon
        K = 0
        if spheres is not None:
            K = self._spheres(spheres, suf)
        motion = () if sphere_vel is None else self._sphere_vel(sphere_vel, sphere_t0, K, suf)
        slab = ()
        if tracks is not None:
            per_problem = getattr(tracks, "ndim", 0) == 4
            Kt = self._tracks(tracks, (ld,) if per_problem else (), N, K, suf)
            slab = (self.be.ptr(tracks if Kt else None), Kt, 4 * N * Kt if per_problem else 0)
        if out is not None:
            U_out, cost, trace, keys = out
        else:
            U_out = U_out if U_out is not None else self.be.empty((3 * N, ld), suf)
            cost = self.be.empty((ld,), suf)
            trace = self.be.empty((max(int(iters), 1), ld), suf) if want_trace else None
            keys = self.be.empty((ld,), "i64") if want_keys else None
        self.lib.call(base, suf, self._B(ld, B), ld, int(n_samples), int(iters), float(sigma), float(temperature), int(seed) & 0xFFFFFFFFFFFFFFFF,
                      int(iter_base) & 0xFFFFFFFF, self.be.ptr(iter_offset), int(index_base) & 0xFFFFFFFF, self.be.ptr(p0), self.be.ptr(v0),
                      self.be.ptr(goal if params.has_goal else None), self.be.ptr(U), self.be.ptr(U_out), self.be.ptr(spheres if K else None), *motion, K,
                      *slab, float(obstacle_weight), self.be.ptr(cost), self.be.ptr(trace), self.be.ptr(keys), *tail, self.be.stream(),
                      params=params)
        return dict(U=U_out, cost=cost, trace=trace if (trace is None or iters > 0) else trace[:0], keys=keys)

    def mppi(self, params: Params, p0, v0, goal, U, n_samples: int, iters: int, sigma: float, temperature: float, seed: int = 0,
             iter_base: int = 0, index_base: int = 0, spheres=None, obstacle_weight: float = 0.0, U_out=None, want_trace: bool = True,
             want_keys: bool = True, iter_offset=None, B: Optional[int] = None, out=None, sphere_vel=None, sphere_t0: float = 0.0):
        """`iters` MPPI iterations of every problem in ONE launch (``se3mpc_mppi_*``, one workgroup per problem): perturb the nominal U
        (3N, ld) with Philox normals of std `sigma`, roll the `n_samples` samples out, weight by exp(-(cost - min) / temperature) and move U
        to the weighted mean.  p0, v0, goal: (3, ld); spheres: (K, 4) rows (cx, cy, cz, r), same dtype, shared by all problems.
        -> dict(U (3N, ld), cost (ld,) with the penalty at U, trace (iters, ld) | None = the minimum sample cost per iteration,
        keys int64 (ld,) | None = the argmin key of each problem's cost).  U_out may be U (in place); iter_offset: int32 (1,) device
        word added to iter_base (graph replays); ``out`` = (U_out, cost, trace, keys) reuses preallocated outputs.
        sphere_vel: None, or (K, 3) rows (vx, vy, vz), same dtype: the spheres move with constant velocity and step k is penalised against
        the centres at sphere_t0 + k dt seconds after the time the table holds (``se3mpc_mppi_moving_*``; keep sphere_t0 small, the kernel
        rounds the time to its own type)."""
        if sphere_vel is not None:
            return self._mppi_call("mppi_moving", (), params, p0, v0, goal, U, n_samples, iters, sigma, temperature, seed, iter_base,
                                   index_base, spheres, obstacle_weight, U_out, want_trace, want_keys, iter_offset, B, out, sphere_vel, sphere_t0)
        return self._mppi_call("mppi", (), params, p0, v0, goal, U, n_samples, iters, sigma, temperature, seed, iter_base,
                               index_base, spheres, obstacle_weight, U_out, want_trace, want_keys, iter_offset, B, out)

    def mppi_tracks(self, params: Params, p0, v0, goal, U, n_samples: int, iters: int, sigma: float, temperature: float, tracks, seed: int = 0,
                    iter_base: int = 0, index_base: int = 0, spheres=None, obstacle_weight: float = 0.0, U_out=None, want_trace: bool = True,
                    want_keys: bool = True, iter_offset=None, B: Optional[int] = None, out=None, sphere_vel=None, sphere_t0: float = 0.0):
        """``se3mpc_mppi_tracks_*``: :meth:`mppi` around moving spheres (sphere_vel None: they stand still) and, behind them, spheres with a
        predicted path.  tracks: (N, Kt, 4) rows (x, y, z, r) shared by all problems, or (ld, N, Kt, 4) one slab per problem, same dtype:
        row [k][j] is tracked sphere j at the time of the state before step k (sphere_t0 + k dt on the table's clock).  Kt = 0 is the
        moving entry.  -> the dict of :meth:`mppi`."""
        suf = self.be.suffix(U)
        K = 0 if spheres is None else spheres.shape[0]
        if sphere_vel is None:
            sphere_vel = self.be.empty((K, 3), suf)
            sphere_vel[...] = 0.0
        return self._mppi_call("mppi_tracks", (), params, p0, v0, goal, U, n_samples, iters, sigma, temperature, seed, iter_base, index_base,
                               spheres, obstacle_weight, U_out, want_trace, want_keys, iter_offset, B, out, sphere_vel, sphere_t0, tracks)

    def mppi_split_workspace(self, params: Params, nprob: int, splits: int):
        """A workspace for :meth:`mppi_split` over `nprob` problems (float64 words; no initialisation needed)."""
        return self.be.empty((max(self.lib.mppi_split_workspace_bytes(params.horizon, int(nprob), int(splits)) // 8, 1),), "f64")

    def mppi_split(self, params: Params, p0, v0, goal, U, n_samples: int, iters: int, sigma: float, temperature: float, splits: int,
                   seed: int = 0, iter_base: int = 0, index_base: int = 0, spheres=None, obstacle_weight: float = 0.0, U_out=None,
                   want_trace: bool = True, want_keys: bool = True, iter_offset=None, B: Optional[int] = None, out=None, workspace=None):
        """:meth:`mppi` with every problem's samples split over `splits` workgroups (``se3mpc_mppi_split_*``): `iters` + 1 launches, one
        per iteration and one that finishes, so that one problem -- or a few -- uses many compute units.  Same operands, keywords and
        returned dict as :meth:`mppi`; `n_samples` must be a multiple of 64 * `splits`.  The partial sums of the splits are folded in
        split order, so the result differs from :meth:`mppi` in the last bits of the float64 sums only (``splits`` = 1: not at all).
        ``workspace``: a float64 tensor of :meth:`mppi_split_workspace` to reuse (required under graph capture); None allocates one."""
        ws = workspace
        if ws is None:
            self.be.check(U, "U")
            ws = self.mppi_split_workspace(params, self._B(U.shape[1], B), splits)
        else:
            self.be.check(ws, "workspace")
            if self.be.suffix(ws) != "f64":
                raise ValueError("workspace: expected a float64 tensor of Ops.mppi_split_workspace")
        tail = (int(splits), self.be.ptr(ws), int(np.prod(ws.shape)) * 8)
        return self._mppi_call("mppi_split", tail, params, p0, v0, goal, U, n_samples, iters, sigma, temperature, seed, iter_base, index_base,
                               spheres, obstacle_weight, U_out, want_trace, want_keys, iter_offset, B, out)

    def mppi_samples(self, params: Params, U, n_samples: int, sigma: float, seed: int = 0, iter_base: int = 0, index_base: int = 0,
                     want_noise: bool = False, want_raw: bool = False, B: Optional[int] = None):
        """The samples of ONE MPPI iteration (g = iter_base) materialised (``se3mpc_mppi_samples_*``): U (3N, ld) ->
        dict(T (3N, S * nprob): column p * S + s = sample s of problem p, noise (3N, S * nprob) | None = its normals,
        raw int32 (4N, S * nprob) | None = its Philox words (read them as uint32))."""
        suf, ld = self._mppi_operands(params, U)
        N, nB, S = params.horizon, self._B(ld, B), int(n_samples)
        cols = max(S * nB, 1)
        T = self.be.empty((3 * N, cols), suf)
        noise = self.be.empty((3 * N, cols), suf) if want_noise else None
        raw = self.be.empty((4 * N, cols), "i32") if want_raw else None
        self.lib.call("mppi_samples", suf, nB, ld, S, float(sigma), int(seed) & 0xFFFFFFFFFFFFFFFF, int(iter_base) & 0xFFFFFFFF,
                      int(index_base) & 0xFFFFFFFF, self.be.ptr(U), self.be.ptr(T), cols, self.be.ptr(noise), self.be.ptr(raw), self.be.stream(),
                      params=params)
        return dict(T=T, noise=noise, raw=raw)

    def spheres_from_grid(self, positions, occupancy, threshold: float = 0.6, target: int = 20, radius: float = 1.0,
                          cap: int = 64):
        """Occupancy grid -> sphere table on the device (f-2).  positions (M, 3), occupancy (M,) in the
        mapper's grid order.  -> (spheres (cap, 4), count int32 (1,)); rows >= count are unspecified."""
        self.be.check(positions, "positions"); self.be.check(occupancy, "occupancy")
        M = occupancy.shape[0]
        if tuple(positions.shape) != (M, 3):
            raise ValueError(f"positions: expected ({M}, 3), got {tuple(positions.shape)}")
        suf = self.be.suffix(positions)
        if self.be.suffix(occupancy) != suf:
            raise ValueError("positions and occupancy must share a dtype")
        spheres = self.be.empty((cap, 4), suf)
        count = self.be.empty((1,), "i32")
        self.lib.call("spheres_from_grid", suf, self.be.ptr(positions), self.be.ptr(occupancy), M, float(threshold),
                      int(target), float(radius), self.be.ptr(spheres), cap, self.be.ptr(count), self.be.stream())
        return spheres, count

    def transpose(self, a):
        """(rows, cols) -> (cols, rows), through the LDS-tiled kernel."""
        self.be.check(a, "a")
        if a.ndim != 2:
            raise ValueError("transpose: 2-D only")
        suf = self.be.suffix(a)
        rows, cols = a.shape
        out = self.be.empty((cols, rows), suf)
        self.lib.call("transpose", suf, rows, cols, self.be.ptr(a), cols, self.be.ptr(out), rows, self.be.stream())
        return out

    # ------------------------------------------------------------------ consumer side of the contract (per-drone rows)
    def controller_state(self, cp: ControllerParams, B: int):
        """Fresh controller members for B drones (GeometricController.__init__ / reset): float64 (B, 12)."""
        st = self.be.empty((B, CONTROLLER_STATE_WORDS), "f64")
        self.lib.controller_reset(cp, B, self.be.ptr(st), self.be.stream())
        return st

    # The operands of the per-drone entry points.  Every front end below composes these, so a tensor of the wrong shape or dtype is a
    # ValueError before any launch and never a pointer a kernel strides over.
    def _ctrl_state(self, state, B):
        """The controller records of B drones: float64 (B, 12)."""
        self.be.check(state, "state")
        if tuple(state.shape) != (B, CONTROLLER_STATE_WORDS) or self.be.suffix(state) != "f64":
            raise ValueError(f"state: float64 ({B}, {CONTROLLER_STATE_WORDS})")

    def _smoother_record(self, state, B):
        self.be.check(state, "smoother state")
        if tuple(state.shape) != (B, SMOOTHER_STATE_WORDS) or self.be.suffix(state) != "f64":
            raise ValueError(f"smoother state: float64 ({B}, {SMOOTHER_STATE_WORDS})")

    def _clock(self, now, B, name="now"):
        self.be.check(now, name)
        if tuple(now.shape) != (B,) or self.be.suffix(now) != "f64":
            raise ValueError(f"{name}: float64 ({B},)")

    def _wind(self, wind, B, suf) -> int:
        """A wind operand: None, one (3,) vector for all drones or (B, 3) rows, of the call's dtype -> its row stride."""
        if wind is None:
            return 0
        self.be.check(wind, "wind")
        if self.be.suffix(wind) != suf or tuple(wind.shape) not in ((3,), (B, 3)):
            raise ValueError(f"wind: (3,) or ({B}, 3) {suf}, got {tuple(wind.shape)}")
        return 3 if wind.ndim == 2 else 0

    def _rows3(self, a, B, name, suf=None):
        self.be.check(a, name)
        if tuple(a.shape) != (B, 3) or (suf is not None and self.be.suffix(a) != suf):
            raise ValueError(f"{name}: expected ({B}, 3) {suf or ''}, got {tuple(a.shape)}")
        return a

    def _drone_state(self, B, suf, pos, vel, att, omega, **more):
        """The four (B, 3) state arrays of B drones (and any further (B, 3) rows by name; None is skipped)."""
        for nm, a in dict(pos=pos, vel=vel, att=att, omega=omega, **more).items():
            if a is not None:
                self._rows3(a, B, nm, suf)

    def _per_drone(self, B, suf, **named):
        """One value per drone: (B,) of the call's dtype; None is skipped."""
        for nm, a in named.items():
            if a is not None:
                self.be.check(a, nm)
                if tuple(a.shape) != (B,) or self.be.suffix(a) != suf:
                    raise ValueError(f"{nm}: expected ({B},) {suf}, got {tuple(a.shape)}")

    @staticmethod
    def _gust(gust):
        """gust = None or (step, (wx, wy, wz)) -> the (gust_step, gust_wind) arguments."""
        if gust is None:
            return -1, None
        return int(gust[0]), (_C.c_double * 3)(*[float(x) for x in gust[1]])

    def _loop_logs(self, nsteps, B, suf, log, target=False):
        """The per-step logs of the loop kernels -> {} or dict(log_state (nsteps, B, 12), log_cmd (nsteps, B, 4), log_time (nsteps, B)[, log_target (nsteps, B, 9)])."""
        if not log:
            return {}
        logs = dict(log_state=self.be.empty((nsteps, B, 12), suf), log_cmd=self.be.empty((nsteps, B, 4), suf), log_time=self.be.empty((nsteps, B), "f64"))
        if target:
            logs["log_target"] = self.be.empty((nsteps, B, 9), suf)
        return logs

    def _plan_ptrs(self, B, suf, timestamps, P, V, A, strides):
        """A plan operand -> the nine plan arguments (N, timestamps, ts_stride, P, strideP, V, strideV, A, strideA) of every entry point that takes one."""
        self.be.check(timestamps, "timestamps")
        if self.be.suffix(timestamps) != "f64":
            raise ValueError("timestamps are float64")
        N = timestamps.shape[-1]
        ts_stride = N if timestamps.ndim == 2 else 0
        if timestamps.ndim == 2 and timestamps.shape[0] != B:
            raise ValueError("timestamps: (N,) or (B, N)")
        if strides is None:
            def st_of(a, nm):
                if a is None:
                    return 0
                self.be.check(a, nm)
                if self.be.suffix(a) != suf or a.ndim not in (2, 3) or a.shape[-2:] != (N, 3) or (a.ndim == 3 and a.shape[0] != B):
                    raise ValueError(f"{nm}: expected ({N}, 3) or ({B}, {N}, 3) {suf}, got {tuple(a.shape)}")
                return 3 * N if a.ndim == 3 else 0
            sP, sV, sA = st_of(P, "P"), st_of(V, "V"), st_of(A, "A")
        else:
            sP, sV, sA = (int(x) for x in strides)
            if hasattr(self.be, "elements_from"):              # explicit strides read past the views' own shapes: check the storage instead
                for a, st, nm in ((P, sP, "P"), (V, sV, "V"), (A, sA, "A")):
                    if a is not None and (st < 0 or (B - 1) * st + 3 * N > self.be.elements_from(a)):
                        raise ValueError(f"{nm}: stride {st} x {B} plans of {N} rows runs past the tensor's storage")
        return [N, self.be.ptr(timestamps), ts_stride, self.be.ptr(P), sP, self.be.ptr(V), sV, self.be.ptr(A), sA]

    def _command_outputs(self, B, suf, want_body_rate):
        """thrust (B,), torque (B, 3), flags int32 (B,)[, body_thrust (B,), body_rates (B, 3)] of a control call -> (dict, their five pointers)."""
        out = dict(thrust=self.be.empty((B,), suf), torque=self.be.empty((B, 3), suf), flags=self.be.empty((B,), "i32"))
        if want_body_rate:
            out.update(body_thrust=self.be.empty((B,), suf), body_rates=self.be.empty((B, 3), suf))
        return out, [self.be.ptr(out.get(k)) for k in ("thrust", "torque", "body_thrust", "body_rates", "flags")]

    def control(self, cp: ControllerParams, state, time, pos, vel, att, omega, dpos, dvel, dacc=None, yaw=None, yaw_rate=None,
                want_body_rate: bool = False):
        """compute_control (+ compute_body_rate_command) for B drones.  time: float64 (B,); pos .. dvel, dacc: (B, 3);
        yaw, yaw_rate: (B,) or None (0).  `state` (B, 12) float64 is updated in place.
        -> dict(thrust (B,), torque (B,3), flags int32 (B,)[, body_thrust (B,), body_rates (B,3)])."""
        B = time.shape[0]
        suf = self.be.suffix(pos)
        self._drone_state(B, suf, pos, vel, att, omega, dpos=dpos, dvel=dvel, dacc=dacc)
        self._per_drone(B, suf, yaw=yaw, yaw_rate=yaw_rate)
        self._clock(time, B, "time")
        self._ctrl_state(state, B)
        out, out_ptrs = self._command_outputs(B, suf, want_body_rate)
        self.lib.loop_call("control", suf, cp, B, self.be.ptr(time), self.be.ptr(pos), self.be.ptr(vel), self.be.ptr(att),
                           self.be.ptr(omega), self.be.ptr(dpos), self.be.ptr(dvel), self.be.ptr(dacc), self.be.ptr(yaw),
                           self.be.ptr(yaw_rate), self.be.ptr(state), *out_ptrs, self.be.stream())
        return out

    def control_fast(self, cp: ControllerParams, state, dt: float, pos, vel, att, omega, dpos, dvel, dacc=None, yaw=None, yaw_rate=None,
                     vehicle_mass: float = 1.0, vehicle_gravity: float = 9.80665):
        """compute_control_fast / compute_control_from_fast_state (controller.py:253-411, :728-768) for B drones: dt in seconds is given;
        vehicle_mass / vehicle_gravity = get_control_constants() (common/vehicle_params.py:19-23 by default).  `state` (B, 12) float64
        is the record se3mpc_control_* uses, updated in place.  -> dict(thrust (B,), torque (B,3), flags int32 (B,))."""
        B = pos.shape[0]
        suf = self.be.suffix(pos)
        self._drone_state(B, suf, pos, vel, att, omega, dpos=dpos, dvel=dvel, dacc=dacc)
        self._per_drone(B, suf, yaw=yaw, yaw_rate=yaw_rate)
        self._ctrl_state(state, B)
        out, (thrust, torque, _, _, flags) = self._command_outputs(B, suf, False)
        self.lib.loop_call("control_fast", suf, cp, float(vehicle_mass), float(vehicle_gravity), B, float(dt), self.be.ptr(pos), self.be.ptr(vel),
                           self.be.ptr(att), self.be.ptr(omega), self.be.ptr(dpos), self.be.ptr(dvel), self.be.ptr(dacc), self.be.ptr(yaw),
                           self.be.ptr(yaw_rate), self.be.ptr(state), thrust, torque, flags, self.be.stream())
        return out

    def monte_carlo(self, params: Params, cp: ControllerParams, sp: SimulatorParams, state, time, pos, vel, att, omega, goal, cycles: int,
                    substeps: int, sim_dt: float, wind=None, want_last_plan: bool = False):
        """se3mpc_monte_carlo_*: `cycles` x (solve from the drone's own state, `substeps` control + simulator steps against the fresh plan) for B
        drones in ONE launch, in place on (state, time, pos, vel, att, omega).  -> dict(overflowed: int32 (1,) device array -- not 0 means
        a solve needed more L-BFGS pairs than the launch's LDS image holds and the run must be repeated with solve + closed_loop launches;
        x, accelerations, info of the last cycle's plan if asked for)."""
        B = pos.shape[0]
        suf = self.be.suffix(pos)
        self._drone_state(B, suf, pos, vel, att, omega, goal=goal)
        self._ctrl_state(state, B)
        self._clock(time, B, "time")
        w_stride = self._wind(wind, B, suf)
        N = params.horizon
        over = self.be.empty((1,), "i32")
        X = self.be.empty((B, 9 * N), suf) if want_last_plan else None
        acc = self.be.empty((B, N, 3), suf) if want_last_plan else None
        info = self.be.empty((B * INFO_DTYPE.itemsize,), "u8") if want_last_plan else None
        self.lib.loop_call("monte_carlo", suf, params, cp, sp, B, int(cycles), int(substeps), float(sim_dt), self.be.ptr(goal), self.be.ptr(wind), w_stride,
                           self.be.ptr(time), self.be.ptr(pos), self.be.ptr(vel), self.be.ptr(att), self.be.ptr(omega), self.be.ptr(state),
                           self.be.ptr(X), self.be.ptr(acc), self.be.ptr(info), self.be.ptr(over), self.be.stream())
        return dict(overflowed=over, x=X, accelerations=acc, info=info)

    def monte_carlo_staged(self, params: Params, cp: ControllerParams, sp: SimulatorParams, state, time, pos, vel, att, omega, goal, cycles: int,
                           substeps: int, sim_dt: float, wind=None, want_last_plan: bool = False, smoother: SmootherParams = None,
                           smoother_state=None, mixer: MixerParams = None, mixer_state=None, motor_health=None):
        """se3mpc_monte_carlo_staged_*: :meth:`monte_carlo` with the reference's TrajectorySmoother between plan and controller (`smoother`
        and `smoother_state` (B, 25)) and / or its MotorMixer and motor model behind the controller (`mixer` and `mixer_state` (B, 5);
        motor_health None, (4,) or (B, 4)), still ONE launch, in place on the records too.  Without both stages it is :meth:`monte_carlo`.
        -> dict(overflowed, x, accelerations, info) as :meth:`monte_carlo`."""
        B = pos.shape[0]
        suf = self.be.suffix(pos)
        self._drone_state(B, suf, pos, vel, att, omega, goal=goal)
        self._ctrl_state(state, B)
        self._clock(time, B, "time")
        if (smoother is None) != (smoother_state is None):
            raise ValueError("monte_carlo_staged: smoother and smoother_state come together or not at all")
        if (mixer is None) != (mixer_state is None):
            raise ValueError("monte_carlo_staged: mixer and mixer_state come together or not at all")
        if motor_health is not None and mixer is None:
            raise ValueError("monte_carlo_staged: motor_health needs mixer")
        if smoother_state is not None:
            self._smoother_record(smoother_state, B)
        if mixer_state is not None:
            self._mixer_record(mixer_state, B)
        h_stride = self._health(motor_health, B, suf)
        w_stride = self._wind(wind, B, suf)
        N = params.horizon
        over = self.be.empty((1,), "i32")
        X = self.be.empty((B, 9 * N), suf) if want_last_plan else None
        acc = self.be.empty((B, N, 3), suf) if want_last_plan else None
        info = self.be.empty((B * INFO_DTYPE.itemsize,), "u8") if want_last_plan else None
        self.lib.loop_call("monte_carlo_staged", suf, params, cp, sp, smoother, mixer, B, int(cycles), int(substeps), float(sim_dt), self.be.ptr(goal),
                           self.be.ptr(wind), w_stride, self.be.ptr(time), self.be.ptr(pos), self.be.ptr(vel), self.be.ptr(att), self.be.ptr(omega),
                           self.be.ptr(state), self.be.ptr(smoother_state), self.be.ptr(mixer_state), self.be.ptr(motor_health), h_stride,
                           self.be.ptr(X), self.be.ptr(acc), self.be.ptr(info), self.be.ptr(over), self.be.stream())
        return dict(overflowed=over, x=X, accelerations=acc, info=info)

    def mppi_closed_loop(self, params: Params, cp: ControllerParams, sp: SimulatorParams, state, time, pos, vel, att, omega, goal, U,
                         cycles: int, substeps: int, sim_dt: float, n_samples: int, iters: int, sigma: float, temperature: float,
                         seed: int = 0, cycle_base: int = 0, shift: int = 1, iter_base: int = 0, index_base: int = 0, spheres=None,
                         obstacle_weight: float = 0.0, wind=None, want_trace: bool = True, want_plan: bool = False, clearance=None,
                         want_clearance: bool = True, sphere_vel=None, sphere_t0: float = 0.0, tracks=None):
        """se3mpc_mppi_closed_loop_*: `cycles` x (`iters` MPPI iterations from the drone's own state on its nominal, the plan handed to the
        controller on the chip, `substeps` control + simulator steps, the nominal shifted by `shift` rows) for B drones in ONE launch, in
        place on (state, time, pos, vel, att, omega) and on the nominals U (B, N, 3).  goal (B, 3); spheres (K, 4) rows (cx, cy, cz, r)
        shared by all drones; wind None, (3,) or (B, 3) newtons.  clearance: a (B,) running minimum to continue (updated in place), or None:
        a fresh one at +inf when `want_clearance` and there are spheres.
        -> dict(U (B, N, 3) = the next cycle's starting nominal, cost (B,) at the last cycle's nominal, trace (B, cycles, iters) | None,
        plan_last (B, 3, N, 3) = P, V, A of the last cycle's plan | None, clearance (B,) | None).
        sphere_vel: None, or (K, 3) rows (vx, vy, vz): the spheres move with constant velocity (``se3mpc_mppi_closed_loop_moving_*``);
        sphere_t0: the time of the RUN's start (cycle 0) after the time the table holds, the same in every chained call -- plan and
        clearance take the centres at the time of the step they look at.
        tracks: None, or (cycles, B, N, Kt, 4) rows (x, y, z, r): spheres with a predicted path behind the moving ones, renewed every cycle
        (``se3mpc_mppi_closed_loop_tracks_*``, see :meth:`mppi_closed_loop_tracks`)."""
        B = pos.shape[0]
        suf = self.be.suffix(pos)
        N = params.horizon
        self._drone_state(B, suf, pos, vel, att, omega, goal=goal)
        self._ctrl_state(state, B)
        self._clock(time, B, "time")
        self.be.check(U, "U")
        if tuple(U.shape) != (B, N, 3) or self.be.suffix(U) != suf:
            raise ValueError(f"U: expected ({B}, {N}, 3) {suf}, got {tuple(U.shape)}")
        w_stride = self._wind(wind, B, suf)
        K = 0
        if spheres is not None:
            K = self._spheres(spheres, suf)
        self._per_drone(B, suf, clearance=clearance)
        if clearance is None and want_clearance and K:
            clearance = self.be.empty((B,), suf)
            clearance[...] = float("inf")
        cost = self.be.empty((B,), suf)
        trace = self.be.empty((B, max(int(cycles), 1), max(int(iters), 1)), suf) if want_trace else None
        plan = self.be.empty((B, 3, N, 3), suf) if want_plan else None
        motion = () if sphere_vel is None else self._sphere_vel(sphere_vel, sphere_t0, K, suf)
        slab = ()
        if tracks is not None:
            if sphere_vel is None:
                raise ValueError("tracks come behind a moving table: pass sphere_vel (zeros for spheres that stand still)")
            Kt = self._tracks(tracks, (max(int(cycles), 0), B), N, K, suf)
            slab = (self.be.ptr(tracks if Kt else None), Kt)
        self.lib.loop_call("mppi_closed_loop_tracks" if tracks is not None else "mppi_closed_loop" if sphere_vel is None else "mppi_closed_loop_moving", suf, params, cp, sp, B, int(cycles), int(substeps), float(sim_dt), int(cycle_base) & 0xFFFFFFFF,
                           int(shift), int(n_samples), int(iters), float(sigma), float(temperature), int(seed) & 0xFFFFFFFFFFFFFFFF,
                           int(iter_base) & 0xFFFFFFFF, int(index_base) & 0xFFFFFFFF, self.be.ptr(goal), self.be.ptr(spheres if K else None), *motion, K,
                           *slab, float(obstacle_weight), self.be.ptr(wind), w_stride, self.be.ptr(time), self.be.ptr(pos), self.be.ptr(vel),
                           self.be.ptr(att), self.be.ptr(omega), self.be.ptr(state), self.be.ptr(U), self.be.ptr(cost), self.be.ptr(trace),
                           self.be.ptr(plan), self.be.ptr(clearance), self.be.stream())
        if trace is not None and (cycles <= 0 or iters <= 0):
            trace = trace[:, :max(int(cycles), 0), :max(int(iters), 0)]
        return dict(U=U, cost=cost, trace=trace, plan_last=plan, clearance=clearance)

    def mppi_closed_loop_tracks(self, params: Params, cp: ControllerParams, sp: SimulatorParams, state, time, pos, vel, att, omega, goal, U,
                                cycles: int, substeps: int, sim_dt: float, n_samples: int, iters: int, sigma: float, temperature: float, tracks,
                                spheres=None, sphere_vel=None, **kw):
        """se3mpc_mppi_closed_loop_tracks_*: :meth:`mppi_closed_loop` around moving spheres (sphere_vel None: they stand still) and, behind
        them, Kt spheres with a predicted path.  tracks (cycles, B, N, Kt, 4) rows (x, y, z, r): cycle c of the call of drone b plans around
        slab [c][b], whose row [k][j] is sphere j at the time of the state before step k of that cycle's plan.  The clearance sees the
        moving rows only.  Every other argument and the result are :meth:`mppi_closed_loop`'s."""
        if sphere_vel is None:
            K = 0 if spheres is None else spheres.shape[0]
            sphere_vel = self.be.empty((K, 3), self.be.suffix(pos))
            sphere_vel[...] = 0.0
        return self.mppi_closed_loop(params, cp, sp, state, time, pos, vel, att, omega, goal, U, cycles, substeps, sim_dt, n_samples, iters, sigma,
                                     temperature, spheres=spheres, sphere_vel=sphere_vel, tracks=tracks, **kw)

    def mppi_swarm_workspace(self, B: int, suf: str, horizon: Optional[int] = None):
        """A workspace for :meth:`mppi_closed_loop_swarm` over `B` drones of dtype `suf` ("f32" / "f64"): the two snapshot images (no
        initialisation needed).  horizon: that of the plans, for ``share_plans=True`` (the images carry the intents too)."""
        esz = {"f32": 4, "f64": 8}[suf]
        need = self.lib.mppi_swarm_workspace_bytes(int(B), esz) if horizon is None else self.lib.mppi_swarm_intent_workspace_bytes(int(B), int(horizon), esz)
        return self.be.empty((max(need // esz, 1),), suf)

    def swarm_intent(self, params: Params, pos, vel, U, intent=None):
        """se3mpc_swarm_intent_*: the intent of every drone, (B, N, 3): row [b][k] = the position before step k of the nominal U (B, N, 3)
        rolled out from (pos, vel) (B, 3) with the plan's recurrence -- what a drone shows its mates under ``share_plans=True``."""
        B, N = pos.shape[0], params.horizon
        suf = self.be.suffix(pos)
        for nm, a, shape in (("pos", pos, (B, 3)), ("vel", vel, (B, 3)), ("U", U, (B, N, 3)), ("intent", intent, (B, N, 3))):
            if a is None:
                continue
            self.be.check(a, nm)
            if tuple(a.shape) != shape or self.be.suffix(a) != suf:
                raise ValueError(f"{nm}: expected {shape} {suf}, got {tuple(a.shape)}")
        if intent is None:
            intent = self.be.empty((B, N, 3), suf)
        self.lib.loop_call("swarm_intent", suf, params, B, self.be.ptr(pos), self.be.ptr(vel), self.be.ptr(U), self.be.ptr(intent), self.be.stream())
        return intent

    def mppi_closed_loop_swarm(self, params: Params, cp: ControllerParams, sp: SimulatorParams, state, time, pos, vel, att, omega, goal, U,
                               cycles: int, substeps: int, sim_dt: float, n_samples: int, iters: int, sigma: float, temperature: float,
                               swarm_size: int = 1, neighbours: int = 0, mate_radius: float = 0.0, seed: int = 0, cycle_base: int = 0,
                               shift: int = 1, iter_base: int = 0, index_base: int = 0, spheres=None, obstacle_weight: float = 0.0, wind=None,
                               want_trace: bool = True, want_plan: bool = False, clearance=None, want_clearance: bool = True, sphere_vel=None,
                               sphere_t0: float = 0.0, separation=None, want_neighbours: bool = False, workspace=None, share_plans: bool = False):
        """se3mpc_mppi_closed_loop_swarm_*: :meth:`mppi_closed_loop` around moving spheres for B / `swarm_size` swarms of `swarm_size`
        drones, every drone planning around its `neighbours` nearest swarm-mates as spheres of radius `mate_radius` that fly on with the
        velocity they have when the cycle starts; one launch per cycle plus a seed, all enqueued by one call.  spheres / sphere_vel: the
        shared table (K, 4) / (K, 3) (sphere_vel None: the spheres stand still).  separation: a (B,) running minimum to continue, or None: a
        fresh one at +inf; it takes the distance to the nearest mate at every cycle's start (:meth:`swarm_separation` adds the state as it
        stands).  workspace: a tensor of :meth:`mppi_swarm_workspace` to reuse (required under graph capture); None allocates one.
        share_plans: the mates are shown as their PLANS (``se3mpc_mppi_closed_loop_swarm_intent_*``): every drone publishes the rollout of
        its nominal beside its snapshot row and a mate's sphere is where that rollout puts it at every step of the horizon, not where its
        velocity points; `neighbours` <= SE3MPC_MAX_TRACKS, and a workspace of ``mppi_swarm_workspace(B, suf, horizon)``.
        -> the dict of :meth:`mppi_closed_loop` plus separation (B,) and neighbours (B, `neighbours`) int32 | None: the drones chosen in
        the last cycle, rank order, -1 in unused slots."""
        B = pos.shape[0]
        suf = self.be.suffix(pos)
        N = params.horizon
        self._drone_state(B, suf, pos, vel, att, omega, goal=goal)
        self._ctrl_state(state, B)
        self._clock(time, B, "time")
        self.be.check(U, "U")
        if tuple(U.shape) != (B, N, 3) or self.be.suffix(U) != suf:
            raise ValueError(f"U: expected ({B}, {N}, 3) {suf}, got {tuple(U.shape)}")
        w_stride = self._wind(wind, B, suf)
        K = 0
        if spheres is not None:
            K = self._spheres(spheres, suf)
        if sphere_vel is None and K:
            sphere_vel = self.be.empty((K, 3), suf)
            sphere_vel[...] = 0.0
        motion = self._sphere_vel(sphere_vel, sphere_t0, K, suf) if K else (None, float(sphere_t0))
        self._per_drone(B, suf, clearance=clearance, separation=separation)
        if clearance is None and want_clearance and K:
            clearance = self.be.empty((B,), suf)
            clearance[...] = float("inf")
        if separation is None:
            separation = self.be.empty((B,), suf)
            separation[...] = float("inf")
        Kn = int(neighbours)
        esz = {"f32": 4, "f64": 8}[suf]
        if workspace is None:
            workspace = self.mppi_swarm_workspace(B, suf, N if share_plans else None)
        else:
            self.be.check(workspace, "workspace")
            if self.be.suffix(workspace) != suf:
                raise ValueError(f"workspace: expected {suf}")
        cost = self.be.empty((B,), suf)
        trace = self.be.empty((B, max(int(cycles), 1), max(int(iters), 1)), suf) if want_trace else None
        plan = self.be.empty((B, 3, N, 3), suf) if want_plan else None
        nb = self.be.empty((B, max(Kn, 1)), "i32") if want_neighbours else None
        if nb is not None:
            nb[...] = -1
        self.lib.loop_call("mppi_closed_loop_swarm_intent" if share_plans else "mppi_closed_loop_swarm", suf, params, cp, sp, B, int(swarm_size), Kn, float(mate_radius), int(cycles), int(substeps),
                           float(sim_dt), int(cycle_base) & 0xFFFFFFFF, int(shift), int(n_samples), int(iters), float(sigma), float(temperature),
                           int(seed) & 0xFFFFFFFFFFFFFFFF, int(iter_base) & 0xFFFFFFFF, int(index_base) & 0xFFFFFFFF, self.be.ptr(goal),
                           self.be.ptr(spheres if K else None), *motion, K, float(obstacle_weight), self.be.ptr(wind), w_stride, self.be.ptr(time),
                           self.be.ptr(pos), self.be.ptr(vel), self.be.ptr(att), self.be.ptr(omega), self.be.ptr(state), self.be.ptr(U),
                           self.be.ptr(cost), self.be.ptr(trace), self.be.ptr(plan), self.be.ptr(clearance), self.be.ptr(separation),
                           self.be.ptr(nb), self.be.ptr(workspace), int(workspace.numel()) * esz, self.be.stream())
        if trace is not None and (cycles <= 0 or iters <= 0):
            trace = trace[:, :max(int(cycles), 0), :max(int(iters), 0)]
        if nb is not None:
            nb = nb[:, :max(Kn, 0)]
        return dict(U=U, cost=cost, trace=trace, plan_last=plan, clearance=clearance, separation=separation, neighbours=nb)

    def swarm_separation(self, pos, vel, swarm_size: int, separation=None):
        """se3mpc_swarm_separation_*: separation[b] = min(separation[b], the distance of drone b to its nearest swarm-mate with a finite
        (pos, vel)) on pos, vel (B, 3) as they stand, swarms of `swarm_size` consecutive drones.  separation None: a fresh (B,) at +inf.
        -> separation."""
        B = pos.shape[0]
        suf = self.be.suffix(pos)
        for nm, a in (("pos", pos), ("vel", vel)):
            self.be.check(a, nm)
            if tuple(a.shape) != (B, 3) or self.be.suffix(a) != suf:
                raise ValueError(f"{nm}: expected ({B}, 3) {suf}, got {tuple(a.shape)}")
        self._per_drone(B, suf, separation=separation)
        if separation is None:
            separation = self.be.empty((B,), suf)
            separation[...] = float("inf")
        self.lib.loop_call("swarm_separation", suf, B, int(swarm_size), self.be.ptr(pos), self.be.ptr(vel), self.be.ptr(separation), self.be.stream())
        return separation

    def mppi_closed_loop_staged(self, params: Params, cp: ControllerParams, sp: SimulatorParams, state, time, pos, vel, att, omega, goal, U,
                                cycles: int, substeps: int, sim_dt: float, n_samples: int, iters: int, sigma: float, temperature: float,
                                seed: int = 0, cycle_base: int = 0, shift: int = 1, iter_base: int = 0, index_base: int = 0, spheres=None,
                                obstacle_weight: float = 0.0, wind=None, want_trace: bool = True, want_plan: bool = False, clearance=None,
                                want_clearance: bool = True, smoother: SmootherParams = None, smoother_state=None, mixer: MixerParams = None,
                                mixer_state=None, motor_health=None, followed=None):
        """se3mpc_mppi_closed_loop_staged_*: :meth:`mppi_closed_loop` with the reference's TrajectorySmoother between plan and controller
        (`smoother` and `smoother_state` (B, 25)) and / or its MotorMixer and motor model behind the controller (`mixer` and `mixer_state`
        (B, 5); motor_health None, (4,) or (B, 4)), still ONE launch and still with the clearance, in place on the records too.  followed:
        (B, 9) = (pos, vel, acc) of the plan each drone follows at the clock the next update_trajectory runs at, updated in place so that a
        later call (with `cycle_base`) continues the run; None: zeros = nothing followed yet (with a smoother).  Without both stages it is
        :meth:`mppi_closed_loop`.  -> what :meth:`mppi_closed_loop` returns, plus followed (None without a smoother)."""
        B = pos.shape[0]
        suf = self.be.suffix(pos)
        N = params.horizon
        self._drone_state(B, suf, pos, vel, att, omega, goal=goal)
        self._ctrl_state(state, B)
        self._clock(time, B, "time")
        self.be.check(U, "U")
        if tuple(U.shape) != (B, N, 3) or self.be.suffix(U) != suf:
            raise ValueError(f"U: expected ({B}, {N}, 3) {suf}, got {tuple(U.shape)}")
        if (smoother is None) != (smoother_state is None):
            raise ValueError("mppi_closed_loop_staged: smoother and smoother_state come together or not at all")
        if (mixer is None) != (mixer_state is None):
            raise ValueError("mppi_closed_loop_staged: mixer and mixer_state come together or not at all")
        if motor_health is not None and mixer is None:
            raise ValueError("mppi_closed_loop_staged: motor_health needs mixer")
        if smoother_state is not None:
            self._smoother_record(smoother_state, B)
        if mixer_state is not None:
            self._mixer_record(mixer_state, B)
        h_stride = self._health(motor_health, B, suf)
        w_stride = self._wind(wind, B, suf)
        if followed is not None:
            self.be.check(followed, "followed")
            if tuple(followed.shape) != (B, 9) or self.be.suffix(followed) != suf:
                raise ValueError(f"followed: expected ({B}, 9) {suf}, got {tuple(followed.shape)}")
        elif smoother is not None:
            followed = self.be.empty((B, 9), suf)
            followed[...] = 0.0
        K = 0
        if spheres is not None:
            K = self._spheres(spheres, suf)
        self._per_drone(B, suf, clearance=clearance)
        if clearance is None and want_clearance and K:
            clearance = self.be.empty((B,), suf)
            clearance[...] = float("inf")
        cost = self.be.empty((B,), suf)
        trace = self.be.empty((B, max(int(cycles), 1), max(int(iters), 1)), suf) if want_trace else None
        plan = self.be.empty((B, 3, N, 3), suf) if want_plan else None
        self.lib.loop_call("mppi_closed_loop_staged", suf, params, cp, sp, smoother, mixer, B, int(cycles), int(substeps), float(sim_dt),
                           int(cycle_base) & 0xFFFFFFFF, int(shift), int(n_samples), int(iters), float(sigma), float(temperature),
                           int(seed) & 0xFFFFFFFFFFFFFFFF, int(iter_base) & 0xFFFFFFFF, int(index_base) & 0xFFFFFFFF, self.be.ptr(goal),
                           self.be.ptr(spheres if K else None), K, float(obstacle_weight), self.be.ptr(wind), w_stride, self.be.ptr(time),
                           self.be.ptr(pos), self.be.ptr(vel), self.be.ptr(att), self.be.ptr(omega), self.be.ptr(state), self.be.ptr(smoother_state),
                           self.be.ptr(mixer_state), self.be.ptr(motor_health), h_stride, self.be.ptr(followed), self.be.ptr(U), self.be.ptr(cost),
                           self.be.ptr(trace), self.be.ptr(plan), self.be.ptr(clearance), self.be.stream())
        if trace is not None and (cycles <= 0 or iters <= 0):
            trace = trace[:, :max(int(cycles), 0), :max(int(iters), 0)]
        return dict(U=U, cost=cost, trace=trace, plan_last=plan, clearance=clearance, followed=followed)

    def controller_integral_update(self, cp: ControllerParams, state, vel_error, dt: float, saturation=None) -> None:
        """_update_integral_error(vel_error, dt, thrust_saturated, torque_saturated) (controller.py:536-564) for B drones, in place on
        `state`.  saturation: int32 (B,) bit 0 thrust, bits 1..3 torque x/y/z, or None."""
        B = vel_error.shape[0]
        suf = self.be.suffix(vel_error)
        self._rows3(vel_error, B, "vel_error", suf)
        self._ctrl_state(state, B)
        if saturation is not None:
            self.be.check(saturation, "saturation")
            if tuple(saturation.shape) != (B,) or not str(saturation.dtype).endswith("int32"):     # (a float32 (B,) array would be read as flag bits)
                raise ValueError("saturation: int32 (B,)")
        self.lib.loop_call("controller_integral_update", suf, cp, B, self.be.ptr(vel_error), float(dt), self.be.ptr(saturation), self.be.ptr(state),
                           self.be.stream())

    def controller_attitude_torque(self, cp: ControllerParams, state, att, omega, b3_des, yaw=None, yaw_rate=None, inertia=None):
        """_geometric_attitude_control / _fast_geometric_attitude_control (controller.py:643-704, :348-411) for B drones.
        inertia: None (diag of cp.inertia) or a host 3x3.  -> dict(torque (B,3), flags int32 (B,)); `state` takes the unsaturated torques
        and the torque saturation flags."""
        B = att.shape[0]
        suf = self.be.suffix(att)
        for a, nm in ((att, "att"), (omega, "omega"), (b3_des, "b3_des")):
            self._rows3(a, B, nm, suf)
        self._per_drone(B, suf, yaw=yaw, yaw_rate=yaw_rate)
        self._ctrl_state(state, B)
        mat = None
        if inertia is not None:
            m = np.asarray(inertia, dtype=np.float64)
            if m.shape != (3, 3):
                raise ValueError("inertia: a 3x3 matrix")
            mat = (_C.c_double * 9)(*m.reshape(-1))
        torque, flags = self.be.empty((B, 3), suf), self.be.empty((B,), "i32")
        self.lib.loop_call("controller_attitude_torque", suf, cp, B, self.be.ptr(att), self.be.ptr(omega), self.be.ptr(b3_des), self.be.ptr(yaw),
                           self.be.ptr(yaw_rate), mat, self.be.ptr(state), self.be.ptr(torque), self.be.ptr(flags), self.be.stream())
        return dict(torque=torque, flags=flags)

    def controller_desired_frame(self, cp: ControllerParams, yaw_vector, b3_des, current_yaw=None, method: int = -1):
        """_detect_yaw_singularity (controller.py:160-189) + the desired frame: method -1 = as _geometric_attitude_control builds it,
        0..3 = _handle_yaw_singularity with that fallback (:191-252).  -> dict(frame (B,9) = b1|b2|b3, cos_angle (B,), singular int32 (B,))."""
        B = yaw_vector.shape[0]
        suf = self.be.suffix(yaw_vector)
        self._rows3(yaw_vector, B, "yaw_vector", suf); self._rows3(b3_des, B, "b3_des", suf)
        self._per_drone(B, suf, current_yaw=current_yaw)
        frame, ca, sg = self.be.empty((B, 9), suf), self.be.empty((B,), suf), self.be.empty((B,), "i32")
        self.lib.loop_call("controller_desired_frame", suf, cp, B, int(method), self.be.ptr(yaw_vector), self.be.ptr(b3_des), self.be.ptr(current_yaw),
                           self.be.ptr(frame), self.be.ptr(ca), self.be.ptr(sg), self.be.stream())
        return dict(frame=frame, cos_angle=ca, singular=sg)

    def control_plan(self, cp: ControllerParams, state, time, sample_time, pos, vel, att, omega, timestamps, P, V=None, A=None,
                     strides=None, want_body_rate: bool = False, want_target: bool = False):
        """compute_control_from_trajectory / compute_body_rate_from_trajectory for B drones: the target is the plan sampled at
        sample_time (float64 (B,)).  Plans as in :meth:`closed_loop`.  -> dict like :meth:`control` (+ target (B, 9))."""
        B = time.shape[0]
        suf = self.be.suffix(pos)
        self._drone_state(B, suf, pos, vel, att, omega)
        self._clock(time, B, "time"); self._clock(sample_time, B, "sample_time")
        self._ctrl_state(state, B)
        plan = self._plan_ptrs(B, suf, timestamps, P, V, A, strides)
        out, out_ptrs = self._command_outputs(B, suf, want_body_rate)
        if want_target:
            out["target"] = self.be.empty((B, 9), suf)
        self.lib.loop_call("control_plan", suf, cp, B, self.be.ptr(time), self.be.ptr(sample_time), self.be.ptr(pos), self.be.ptr(vel),
                           self.be.ptr(att), self.be.ptr(omega), *plan, self.be.ptr(state), *out_ptrs, self.be.ptr(out.get("target")), self.be.stream())
        return out

    def simulator_step(self, sp: SimulatorParams, time, pos, vel, att, omega, thrust, torque, dt: float, wind=None):
        """DroneSimulator.step for B drones: advances time, pos, vel, att, omega in place.  thrust (B,), torque (B, 3); wind as in
        :meth:`closed_loop`."""
        B = time.shape[0]
        suf = self.be.suffix(pos)
        self._drone_state(B, suf, pos, vel, att, omega, torque=torque)
        self._clock(time, B, "time")
        self._per_drone(B, suf, thrust=thrust)
        w_stride = self._wind(wind, B, suf)
        self.lib.loop_call("simulator_step", suf, sp, B, float(dt), self.be.ptr(thrust), self.be.ptr(torque), self.be.ptr(wind), w_stride,
                           self.be.ptr(time), self.be.ptr(pos), self.be.ptr(vel), self.be.ptr(att), self.be.ptr(omega), self.be.stream())

    def closed_loop(self, cp: ControllerParams, sp: SimulatorParams, state, time, pos, vel, att, omega, timestamps, P, V=None, A=None,
                    nsteps: int = 1, sim_dt: float = 0.01, strides=None, wind=None, gust=None, stop_at_plan_end: bool = True,
                    log: bool = False):
        """`nsteps` x (plan sample -> compute_control -> DroneSimulator.step) for B drones in ONE launch; time, pos, vel, att,
        omega and `state` are updated in place.  Plans: timestamps float64 (N,) shared or (B, N); P, V, A either (N, 3) shared,
        (B, N, 3) per drone, or -- with ``strides=(strideP, strideV, strideA)`` in elements -- views into the solver's outputs
        (P = X, V = X[:, 3N:], A = accelerations).  wind: None, (3,) or (B, 3) newtons; gust = (step, (wx, wy, wz)).
        -> dict(steps_taken int32 (B,)[, log_state (nsteps, B, 12), log_cmd (nsteps, B, 4), log_time (nsteps, B)])."""
        B = time.shape[0]
        suf = self.be.suffix(pos)
        self._drone_state(B, suf, pos, vel, att, omega)
        self._clock(time, B, "time")
        self._ctrl_state(state, B)
        plan = self._plan_ptrs(B, suf, timestamps, P, V, A, strides)
        w_stride = self._wind(wind, B, suf)
        gust_step, gust_vec = self._gust(gust)
        logs = self._loop_logs(nsteps, B, suf, log)
        taken = self.be.empty((B,), "i32")
        self.lib.loop_call("closed_loop", suf, cp, sp, B, int(nsteps), float(sim_dt), *plan, self.be.ptr(time), self.be.ptr(pos),
                           self.be.ptr(vel), self.be.ptr(att), self.be.ptr(omega), self.be.ptr(state), self.be.ptr(wind), w_stride,
                           gust_step, gust_vec, int(bool(stop_at_plan_end)), self.be.ptr(logs.get("log_state")), self.be.ptr(logs.get("log_cmd")),
                           self.be.ptr(logs.get("log_time")), self.be.ptr(taken), self.be.stream())
        return dict(steps_taken=taken, **logs)

    # ------------------------------------------------------------------ TrajectorySmoother (per-drone rows)
    def smoother_state(self, B: int):
        """Fresh smoother members for B drones (TrajectorySmoother.__init__): float64 (B, 25), all zero = no trajectory."""
        st = self.be.empty((B, SMOOTHER_STATE_WORDS), "f64")
        self.lib.smoother_reset(B, self.be.ptr(st), self.be.stream())
        return st

    def smoother_update(self, mp: SmootherParams, state, now, timestamps, P, V=None, A=None, strides=None, old=None, old_strides=None) -> None:
        """update_trajectory for B drones at the clocks now float64 (B,): the new plan (timestamps, P, V, A[, strides]) as in :meth:`closed_loop`
        (N = 0 rows allowed), `old` = None or the (timestamps, P, V, A) the drones have been following (read for drones that have a
        trajectory).  `state` float64 (B, 25) is updated in place."""
        B = now.shape[0]
        self._clock(now, B)
        self._smoother_record(state, B)
        suf = self.be.suffix(P)
        new_args = self._plan_ptrs(B, suf, timestamps, P, V, A, strides)
        old_args = [0, 0, 0, 0, 0, 0, 0, 0, 0] if old is None else self._plan_ptrs(B, suf, old[0], old[1], old[2], old[3], old_strides)
        self.lib.loop_call("smoother_update", suf, mp, B, self.be.ptr(now), *old_args, *new_args, self.be.ptr(state), self.be.stream())

    def smoother_desired(self, mp: SmootherParams, state, now, pos, vel, timestamps, P, V=None, A=None, strides=None):
        """get_desired_state for B drones at the clocks now float64 (B,): pos, vel (B, 3) the drones' own state, the current plan as in
        :meth:`closed_loop` (N = 0 rows allowed).  `state` is updated in place.
        -> dict(target (B, 9) = (position, velocity, acceleration), branch int32 (B,): 0 failsafe, 1 transition point, 2 transition just
        completed, 3 normal following, 4 no trajectory)."""
        B = now.shape[0]
        self._clock(now, B)
        self._smoother_record(state, B)
        suf = self.be.suffix(pos)
        self._rows3(pos, B, "pos", suf); self._rows3(vel, B, "vel", suf)
        plan = self._plan_ptrs(B, suf, timestamps, P, V, A, strides)
        target, branch = self.be.empty((B, 9), suf), self.be.empty((B,), "i32")
        self.lib.loop_call("smoother_desired", suf, mp, B, self.be.ptr(now), self.be.ptr(pos), self.be.ptr(vel), *plan, self.be.ptr(state),
                           self.be.ptr(target), self.be.ptr(branch), self.be.stream())
        return dict(target=target, branch=branch)

    def closed_loop_smoothed(self, mp: SmootherParams, cp: ControllerParams, sp: SimulatorParams, state, smoother_state, time, pos, vel, att,
                             omega, timestamps, P, V=None, A=None, nsteps: int = 1, sim_dt: float = 0.01, strides=None, wind=None, gust=None,
                             log: bool = False):
        """`nsteps` x (get_desired_state -> compute_control -> DroneSimulator.step) for B drones in ONE launch: :meth:`closed_loop` with the
        reference's TrajectorySmoother between plan and controller.  time, pos, vel, att, omega, `state` (B, 12) and `smoother_state`
        (B, 25) are updated in place.  -> dict([log_state (nsteps, B, 12), log_cmd (nsteps, B, 4), log_time (nsteps, B), log_target
        (nsteps, B, 9)])."""
        B = time.shape[0]
        suf = self.be.suffix(pos)
        self._drone_state(B, suf, pos, vel, att, omega)
        self._clock(time, B, "time")
        self._ctrl_state(state, B)
        self._smoother_record(smoother_state, B)
        plan = self._plan_ptrs(B, suf, timestamps, P, V, A, strides)
        w_stride = self._wind(wind, B, suf)
        gust_step, gust_vec = self._gust(gust)
        nsteps = int(nsteps)
        logs = self._loop_logs(nsteps, B, suf, log, target=True)
        self.lib.loop_call("closed_loop_smoothed", suf, mp, cp, sp, B, nsteps, float(sim_dt), *plan, self.be.ptr(time), self.be.ptr(pos),
                           self.be.ptr(vel), self.be.ptr(att), self.be.ptr(omega), self.be.ptr(state), self.be.ptr(smoother_state),
                           self.be.ptr(wind), w_stride, gust_step, gust_vec, self.be.ptr(logs.get("log_state")), self.be.ptr(logs.get("log_cmd")),
                           self.be.ptr(logs.get("log_time")), self.be.ptr(logs.get("log_target")), self.be.stream())
        return logs

    # ------------------------------------------------------------------ latency buffer and OnboardController (per-drone rows)
    def onboard_state(self, B: int):
        """Fresh OnboardController members for B drones (reset()): float64 (B, 14), all zero = last_time None."""
        st = self.be.empty((B, ONBOARD_STATE_WORDS), "f64")
        self.lib.onboard_reset(B, self.be.ptr(st), self.be.stream())
        return st

    def latency_buffer(self, B: int, depth: int, suf: str):
        """An empty DroneStateLatencyBuffer of `depth` slots for B drones -> dict(depth, ring (depth, 12, B) of the precision `suf`, ring_time
        float64 (depth, B), state float64 (B, 4)); depth = 0 -> dict(depth=0, ring=None, ring_time=None, state=None): no buffer.  The
        ring is zero-filled here only so that a copy of it is reproducible; no slot is read before it is written."""
        depth = int(depth)
        if depth == 0:
            return dict(depth=0, ring=None, ring_time=None, state=None)
        if not 1 <= depth <= LATENCY_MAX_DEPTH:
            raise ValueError(f"latency depth: 0 (no buffer) or 1..{LATENCY_MAX_DEPTH}")
        ring, ring_time = self.be.empty((depth, 12, B), suf), self.be.empty((depth, B), "f64")
        ring[...] = 0; ring_time[...] = 0
        st = self.be.empty((B, LATENCY_STATE_WORDS), "f64")
        self.lib.latency_reset(B, depth, self.be.ptr(st), self.be.stream())
        return dict(depth=depth, ring=ring, ring_time=ring_time, state=st)

    def _latency(self, buf, B, suf):
        """A latency_buffer() dict checked against the call -> (depth, ring, ring_time, state) pointers."""
        depth = int(buf["depth"])
        if depth == 0:
            return 0, 0, 0, 0
        if not 1 <= depth <= LATENCY_MAX_DEPTH:
            raise ValueError(f"latency depth: 0 (no buffer) or 1..{LATENCY_MAX_DEPTH}")
        ring, rt, st = buf["ring"], buf["ring_time"], buf["state"]
        for a, nm in ((ring, "ring"), (rt, "ring_time"), (st, "latency state")):
            self.be.check(a, nm)
        if tuple(ring.shape) != (depth, 12, B) or self.be.suffix(ring) != suf:
            raise ValueError(f"ring: ({depth}, 12, {B}) {suf}, got {tuple(ring.shape)}")
        if tuple(rt.shape) != (depth, B) or self.be.suffix(rt) != "f64":
            raise ValueError(f"ring_time: float64 ({depth}, {B})")
        if tuple(st.shape) != (B, LATENCY_STATE_WORDS) or self.be.suffix(st) != "f64":
            raise ValueError(f"latency state: float64 ({B}, {LATENCY_STATE_WORDS})")
        return depth, self.be.ptr(ring), self.be.ptr(rt), self.be.ptr(st)

    def _onboard_record(self, state, B):
        self.be.check(state, "onboard state")
        if tuple(state.shape) != (B, ONBOARD_STATE_WORDS) or self.be.suffix(state) != "f64":
            raise ValueError(f"onboard state: float64 ({B}, {ONBOARD_STATE_WORDS})")

    def latency_push(self, buf, time, pos, vel, att, omega):
        """DroneStateLatencyBuffer.push(state, state.timestamp) for B drones on a latency_buffer() (depth >= 1), updated in place.
        -> dict(time float64 (B,), pos, vel, att, omega (B, 3)): the delayed state (the current one while the buffer fills)."""
        B = time.shape[0]
        suf = self.be.suffix(pos)
        self._drone_state(B, suf, pos, vel, att, omega)
        self._clock(time, B, "time")
        if int(buf["depth"]) < 1:
            raise ValueError("latency_push needs a buffer of depth >= 1")
        depth, ring, rt, st = self._latency(buf, B, suf)
        out = dict(time=self.be.empty((B,), "f64"), pos=self.be.empty((B, 3), suf), vel=self.be.empty((B, 3), suf), att=self.be.empty((B, 3), suf),
                   omega=self.be.empty((B, 3), suf))
        self.lib.loop_call("latency_push", suf, B, depth, self.be.ptr(time), self.be.ptr(pos), self.be.ptr(vel), self.be.ptr(att), self.be.ptr(omega),
                           ring, rt, st, self.be.ptr(out["time"]), self.be.ptr(out["pos"]), self.be.ptr(out["vel"]), self.be.ptr(out["att"]),
                           self.be.ptr(out["omega"]), self.be.stream())
        return out

    _NO_PLAN = [0, 0, 0, 0, 0, 0, 0, 0, 0]          # the nine plan arguments of "no plan": N = 0 rows, NULL pointers

    def onboard_control(self, op: OnboardParams, state, time, pos, att, omega, timestamps=None, P=None, V=None, A=None, strides=None):
        """OnboardController.compute_control_command for B drones: time float64 (B,) = state.timestamp, pos, att, omega (B, 3); the plan as in
        :meth:`closed_loop`, or timestamps = None: no plan -> get_fallback_command with target = pos and `state` untouched.  `state`
        float64 (B, 14) is updated in place.  -> dict(thrust (B,), torque (B, 3), target_pos (B, 3))."""
        B = time.shape[0]
        suf = self.be.suffix(pos)
        self._drone_state(B, suf, pos, None, att, omega)
        self._clock(time, B, "time")
        self._onboard_record(state, B)
        plan = self._NO_PLAN if timestamps is None else self._plan_ptrs(B, suf, timestamps, P, V, A, strides)
        out = dict(thrust=self.be.empty((B,), suf), torque=self.be.empty((B, 3), suf), target_pos=self.be.empty((B, 3), suf))
        self.lib.loop_call("onboard_control", suf, op, B, self.be.ptr(time), self.be.ptr(pos), self.be.ptr(att), self.be.ptr(omega), *plan,
                           self.be.ptr(state), self.be.ptr(out["thrust"]), self.be.ptr(out["torque"]), self.be.ptr(out["target_pos"]), self.be.stream())
        return out

    def edge_loop(self, op: OnboardParams, sp: SimulatorParams, onboard_state, buf, time, pos, vel, att, omega, timestamps=None, P=None, V=None,
                  A=None, nsteps: int = 1, sim_dt: float = 0.01, strides=None, wind=None, gust=None, log: bool = False, zero_thrust_steps=None):
        """`nsteps` x (latency push -> compute_control_command or fallback -> DroneSimulator.step) for B drones in ONE launch: the body of the
        reference's edge loop (edge/main.py:80-95).  buf: a latency_buffer() (depth 0 = none); the plan as in :meth:`closed_loop`, or
        timestamps = None: no plan (the fallback command).  time, pos, vel, att, omega, `onboard_state` (B, 14) and the buffer are updated in
        place; zero_thrust_steps: None or int32 (B,) counters that are incremented.
        -> dict([log_state (nsteps, B, 12), log_cmd (nsteps, B, 4), log_time (nsteps, B), log_target (nsteps, B, 3), log_delayed_time
        (nsteps, B)])."""
        B = time.shape[0]
        suf = self.be.suffix(pos)
        self._drone_state(B, suf, pos, vel, att, omega)
        self._clock(time, B, "time")
        self._onboard_record(onboard_state, B)
        depth, ring, rt, lst = self._latency(buf, B, suf)
        plan = self._NO_PLAN if timestamps is None else self._plan_ptrs(B, suf, timestamps, P, V, A, strides)
        w_stride = self._wind(wind, B, suf)
        gust_step, gust_vec = self._gust(gust)
        nsteps = int(nsteps)
        logs = self._loop_logs(nsteps, B, suf, log)
        if log:
            logs.update(log_target=self.be.empty((nsteps, B, 3), suf), log_delayed_time=self.be.empty((nsteps, B), "f64"))
        if zero_thrust_steps is not None:
            self.be.check(zero_thrust_steps, "zero_thrust_steps")
            if tuple(zero_thrust_steps.shape) != (B,) or zero_thrust_steps.dtype != self.be.empty((0,), "i32").dtype:
                raise ValueError(f"zero_thrust_steps: int32 ({B},)")
        self.lib.loop_call("edge_loop", suf, op, sp, B, nsteps, float(sim_dt), *plan, self.be.ptr(time), self.be.ptr(pos), self.be.ptr(vel),
                           self.be.ptr(att), self.be.ptr(omega), self.be.ptr(onboard_state), depth, ring, rt, lst, self.be.ptr(wind), w_stride,
                           gust_step, gust_vec, self.be.ptr(logs.get("log_state")), self.be.ptr(logs.get("log_cmd")), self.be.ptr(logs.get("log_time")),
                           self.be.ptr(logs.get("log_target")), self.be.ptr(logs.get("log_delayed_time")), self.be.ptr(zero_thrust_steps),
                           self.be.stream())
        return logs

    def monte_carlo_edge(self, params: Params, op: OnboardParams, sp: SimulatorParams, onboard_state, buf, time, pos, vel, att, omega, goal,
                         cycles: int, substeps: int, sim_dt: float, wind=None, first_cycle: int = 0, zero_thrust_steps=None,
                         want_last_plan: bool = False):
        """se3mpc_monte_carlo_edge_*: `cycles` x (solve from the drone's own state, `substeps` steps of :meth:`edge_loop` against the fresh plan)
        for B drones in ONE launch, in place on (onboard_state (B, 14), the latency_buffer() `buf`, time, pos, vel, att, omega);
        zero_thrust_steps: None or int32 (B,) counters that are incremented.  The plan's stamps count from `first_cycle`: a second call with
        first_cycle = the cycles already flown continues a run on the same operands.  -> dict(overflowed, x, accelerations, info) as
        :meth:`monte_carlo` (not 0: repeat the run with solve + edge_loop launches)."""
        B = pos.shape[0]
        suf = self.be.suffix(pos)
        self._drone_state(B, suf, pos, vel, att, omega, goal=goal)
        self._clock(time, B, "time")
        self._onboard_record(onboard_state, B)
        depth, ring, rt, lst = self._latency(buf, B, suf)
        w_stride = self._wind(wind, B, suf)
        if zero_thrust_steps is not None:
            self.be.check(zero_thrust_steps, "zero_thrust_steps")
            if tuple(zero_thrust_steps.shape) != (B,) or zero_thrust_steps.dtype != self.be.empty((0,), "i32").dtype:
                raise ValueError(f"zero_thrust_steps: int32 ({B},)")
        N = params.horizon
        over = self.be.empty((1,), "i32")
        X = self.be.empty((B, 9 * N), suf) if want_last_plan else None
        acc = self.be.empty((B, N, 3), suf) if want_last_plan else None
        info = self.be.empty((B * INFO_DTYPE.itemsize,), "u8") if want_last_plan else None
        self.lib.loop_call("monte_carlo_edge", suf, params, op, sp, B, int(cycles), int(substeps), float(sim_dt), int(first_cycle), self.be.ptr(goal),
                           self.be.ptr(wind), w_stride, self.be.ptr(time), self.be.ptr(pos), self.be.ptr(vel), self.be.ptr(att), self.be.ptr(omega),
                           self.be.ptr(onboard_state), depth, ring, rt, lst, self.be.ptr(zero_thrust_steps), self.be.ptr(X), self.be.ptr(acc),
                           self.be.ptr(info), self.be.ptr(over), self.be.stream())
        out = dict(overflowed=over)
        if want_last_plan:
            out.update(x=X, accelerations=acc, info=info)
        return out

    def mppi_closed_loop_edge(self, params: Params, op: OnboardParams, sp: SimulatorParams, onboard_state, buf, time, pos, vel, att, omega, goal, U,
                              cycles: int, substeps: int, sim_dt: float, n_samples: int, iters: int, sigma: float, temperature: float,
                              seed: int = 0, cycle_base: int = 0, shift: int = 1, iter_base: int = 0, index_base: int = 0, spheres=None,
                              obstacle_weight: float = 0.0, wind=None, want_trace: bool = True, want_plan: bool = False, clearance=None,
                              want_clearance: bool = True, zero_thrust_steps=None):
        """se3mpc_mppi_closed_loop_edge_*: `cycles` x (`iters` MPPI iterations from the drone's own state on its nominal as
        :meth:`mppi_closed_loop`, the plan handed over on the chip, `substeps` steps of :meth:`edge_loop` against it, the nominal shifted by
        `shift` rows) for B drones in ONE launch, in place on (onboard_state (B, 14), the latency_buffer() `buf`, time, pos, vel, att, omega)
        and on the nominals U (B, N, 3); zero_thrust_steps: None or int32 (B,) counters that are added to.  goal, spheres, wind, clearance and
        want_clearance as :meth:`mppi_closed_loop`.  All cross-cycle state is in these operands: a second call with cycle_base = the cycles
        already flown continues a run.
        -> dict(U, cost, trace, plan_last, clearance) as :meth:`mppi_closed_loop`."""
        B = pos.shape[0]
        suf = self.be.suffix(pos)
        N = params.horizon
        self._drone_state(B, suf, pos, vel, att, omega, goal=goal)
        self._clock(time, B, "time")
        self._onboard_record(onboard_state, B)
        depth, ring, rt, lst = self._latency(buf, B, suf)
        self.be.check(U, "U")
        if tuple(U.shape) != (B, N, 3) or self.be.suffix(U) != suf:
            raise ValueError(f"U: expected ({B}, {N}, 3) {suf}, got {tuple(U.shape)}")
        w_stride = self._wind(wind, B, suf)
        K = 0
        if spheres is not None:
            K = self._spheres(spheres, suf)
        self._per_drone(B, suf, clearance=clearance)
        if zero_thrust_steps is not None:
            self.be.check(zero_thrust_steps, "zero_thrust_steps")
            if tuple(zero_thrust_steps.shape) != (B,) or zero_thrust_steps.dtype != self.be.empty((0,), "i32").dtype:
                raise ValueError(f"zero_thrust_steps: int32 ({B},)")
        if clearance is None and want_clearance and K:
            clearance = self.be.empty((B,), suf)
            clearance[...] = float("inf")
        cost = self.be.empty((B,), suf)
        trace = self.be.empty((B, max(int(cycles), 1), max(int(iters), 1)), suf) if want_trace else None
        plan = self.be.empty((B, 3, N, 3), suf) if want_plan else None
        self.lib.loop_call("mppi_closed_loop_edge", suf, params, op, sp, B, int(cycles), int(substeps), float(sim_dt), int(cycle_base) & 0xFFFFFFFF,
                           int(shift), int(n_samples), int(iters), float(sigma), float(temperature), int(seed) & 0xFFFFFFFFFFFFFFFF,
                           int(iter_base) & 0xFFFFFFFF, int(index_base) & 0xFFFFFFFF, self.be.ptr(goal), self.be.ptr(spheres if K else None), K,
                           float(obstacle_weight), self.be.ptr(wind), w_stride, self.be.ptr(time), self.be.ptr(pos), self.be.ptr(vel),
                           self.be.ptr(att), self.be.ptr(omega), self.be.ptr(onboard_state), depth, ring, rt, lst, self.be.ptr(zero_thrust_steps),
                           self.be.ptr(U), self.be.ptr(cost), self.be.ptr(trace), self.be.ptr(plan), self.be.ptr(clearance), self.be.stream())
        if trace is not None and (cycles <= 0 or iters <= 0):
            trace = trace[:, :max(int(cycles), 0), :max(int(iters), 0)]
        return dict(U=U, cost=cost, trace=trace, plan_last=plan, clearance=clearance)

    # ------------------------------------------------------------------ MotorMixer and motor model (per-drone rows)
    def _mixer_record(self, state, B):
        self.be.check(state, "mixer state")
        if tuple(state.shape) != (B, MIXER_STATE_WORDS) or self.be.suffix(state) != "f64":
            raise ValueError(f"mixer state: float64 ({B}, {MIXER_STATE_WORDS})")

    def _rows4(self, a, B, name, suf):
        self.be.check(a, name)
        if tuple(a.shape) != (B, 4) or self.be.suffix(a) != suf:
            raise ValueError(f"{name}: expected ({B}, 4) {suf}, got {tuple(a.shape)}")

    def _health(self, motor_health, B, suf) -> int:
        """A motor_health operand: None, one (4,) row for all drones or (B, 4) rows, of the call's dtype -> its row stride."""
        if motor_health is None:
            return 0
        self.be.check(motor_health, "motor_health")
        if self.be.suffix(motor_health) != suf or tuple(motor_health.shape) not in ((4,), (B, 4)):
            raise ValueError(f"motor_health: (4,) or ({B}, 4) {suf}, got {tuple(motor_health.shape)}")
        return 4 if motor_health.ndim == 2 else 0

    def mixer_state(self, B: int):
        """Fresh mixer members for B drones (MotorMixer.__init__): float64 (B, 5) = saturation_events, last_motor_commands; all zero."""
        st = self.be.empty((B, MIXER_STATE_WORDS), "f64")
        self.lib.mixer_reset(B, self.be.ptr(st), self.be.stream())
        return st

    def mixer_mix(self, mp: MixerParams, thrust, torque, state=None, want_flags: bool = True, want_body_rate: bool = False):
        """mix_commands for B drones: thrust (B,), torque (B, 3) -> dict(pwm (B, 4)[, flags int32 (B,)][, body_rate (B, 4) = (normalised
        thrust, roll, pitch, yaw rate) of _convert_to_body_rate_cmd]).  `state`: None or the records float64 (B, 5), updated in place."""
        B = thrust.shape[0]
        suf = self.be.suffix(thrust)
        self._per_drone(B, suf, thrust=thrust)
        self._rows3(torque, B, "torque", suf)
        if state is not None:
            self._mixer_record(state, B)
        out = dict(pwm=self.be.empty((B, 4), suf))
        if want_flags:
            out["flags"] = self.be.empty((B,), "i32")
        if want_body_rate:
            out["body_rate"] = self.be.empty((B, 4), suf)
        self.lib.loop_call("mixer_mix", suf, mp, B, self.be.ptr(thrust), self.be.ptr(torque), self.be.ptr(state), self.be.ptr(out["pwm"]),
                           self.be.ptr(out.get("flags")), self.be.ptr(out.get("body_rate")), self.be.stream())
        return out

    MIXER_READBACK = ("motor_thrust", "motor_torque", "motor_rpm", "allocation", "wrench")

    def mixer_readback(self, mp: MixerParams, pwm, motor_health=None, want=MIXER_READBACK):
        """What the motors do under pwm (B, 4): each (B, 4) of `want` -- motor_thrust (thrust_from_pwm times the motor's health),
        motor_torque, motor_rpm, allocation (get_control_allocation: the inverse matrix on the motor thrusts) and wrench (B @ motor
        thrusts = the realised (thrust, torque)).  motor_health: None (1), (4,) or (B, 4)."""
        B = pwm.shape[0]
        suf = self.be.suffix(pwm)
        self._rows4(pwm, B, "pwm", suf)
        h_stride = self._health(motor_health, B, suf)
        unknown = [k for k in want if k not in self.MIXER_READBACK]
        if unknown:
            raise ValueError(f"mixer_readback: no output {unknown}")
        out = {k: self.be.empty((B, 4), suf) for k in self.MIXER_READBACK if k in want}
        self.lib.loop_call("mixer_readback", suf, mp, B, self.be.ptr(pwm), self.be.ptr(motor_health), h_stride,
                           *[self.be.ptr(out.get(k)) for k in self.MIXER_READBACK], self.be.stream())
        return out

    def closed_loop_actuated(self, mp: MixerParams, cp: ControllerParams, sp: SimulatorParams, state, mixer_state, time, pos, vel, att, omega,
                             timestamps, P, V=None, A=None, nsteps: int = 1, sim_dt: float = 0.01, strides=None, smoother: SmootherParams = None,
                             smoother_state=None, motor_health=None, wind=None, gust=None, log: bool = False):
        """`nsteps` x (desired state -> compute_control -> mix_commands -> the motors' wrench -> DroneSimulator.step) for B drones in ONE
        launch: :meth:`closed_loop_smoothed` (with `smoother` and `smoother_state`) or the raw plan sample of :meth:`closed_loop` (without
        both), with the simulator under what the motors deliver.  `mixer_state` (B, 5) is updated in place with the other records.
        -> dict([log_state, log_cmd (the COMMAND), log_time, log_target, log_pwm (nsteps, B, 4), log_wrench (nsteps, B, 4)])."""
        B = time.shape[0]
        suf = self.be.suffix(pos)
        self._drone_state(B, suf, pos, vel, att, omega)
        self._clock(time, B, "time")
        self._ctrl_state(state, B)
        self._mixer_record(mixer_state, B)
        if (smoother is None) != (smoother_state is None):
            raise ValueError("closed_loop_actuated: smoother and smoother_state come together or not at all")
        if smoother_state is not None:
            self._smoother_record(smoother_state, B)
        plan = self._plan_ptrs(B, suf, timestamps, P, V, A, strides)
        h_stride = self._health(motor_health, B, suf)
        w_stride = self._wind(wind, B, suf)
        gust_step, gust_vec = self._gust(gust)
        nsteps = int(nsteps)
        logs = self._loop_logs(nsteps, B, suf, log, target=True)
        if log:
            logs.update(log_pwm=self.be.empty((nsteps, B, 4), suf), log_wrench=self.be.empty((nsteps, B, 4), suf))
        self.lib.loop_call("closed_loop_actuated", suf, smoother, cp, sp, mp, B, nsteps, float(sim_dt), *plan, self.be.ptr(time), self.be.ptr(pos),
                           self.be.ptr(vel), self.be.ptr(att), self.be.ptr(omega), self.be.ptr(state), self.be.ptr(smoother_state),
                           self.be.ptr(mixer_state), self.be.ptr(motor_health), h_stride, self.be.ptr(wind), w_stride, gust_step, gust_vec,
                           *[self.be.ptr(logs.get(k)) for k in ("log_state", "log_cmd", "log_time", "log_target", "log_pwm", "log_wrench")],
                           self.be.stream())
        return logs

    # ------------------------------------------------------------------ uncertainty field (mission layer, dense float64 grids)
    def _f64(self, a, shape, name):
        self.be.check(a, name)
        if self.be.suffix(a) != "f64" or tuple(a.shape) != tuple(shape):
            raise ValueError(f"{name}: expected float64 {tuple(shape)}, got {tuple(a.shape)}")
        return a

    def _i32(self, a, min_words, name):
        self.be.check(a, name)
        if a.ndim != 1 or not str(a.dtype).endswith("int32"):
            raise ValueError(f"{name}: expected a flat int32 array, got {a.dtype} {tuple(a.shape)}")
        if a.shape[0] < min_words:
            raise ValueError(f"{name}: {a.shape[0]} words, {min_words} needed")
        return a

    def ufield_desc(self, uncertainty, observation_count, origin, resolution: float) -> UFieldDesc:
        """The descriptor of a field whose two float64 grids (n0, n1, n2) live on the backend; origin = scene_bounds[0]."""
        self.be.check(uncertainty, "uncertainty")
        if uncertainty.ndim != 3:
            raise ValueError(f"uncertainty: expected a 3-D grid, got {tuple(uncertainty.shape)}")
        n = tuple(int(x) for x in uncertainty.shape)
        self._f64(uncertainty, n, "uncertainty")
        self._f64(observation_count, n, "observation_count")
        return UFieldDesc(uncertainty=self.be.ptr(uncertainty), observation_count=self.be.ptr(observation_count), n=(_C.c_int32 * 3)(*n), reserved=0,
                          origin=(_C.c_double * 3)(*[float(v) for v in origin]), resolution=float(resolution))

    def ufield_workspace(self, grid_size, max_regions: int):
        """Zeroed int32 scratch that every ufield_* call accepts for this grid and up to max_regions rows."""
        words = self.lib.ufield_workspace(int(grid_size[0]), int(grid_size[1]), int(grid_size[2]), int(max_regions))
        if words < 0:
            raise ValueError(f"ufield_workspace: grid {tuple(grid_size)} / max_regions {max_regions} refused")
        ws = self.be.empty((words,), "i32")
        ws[...] = 0
        return ws

    def ufield_fill(self, desc: UFieldDesc) -> None:
        self.lib.ufield("fill", desc, self.be.stream())

    def ufield_stamp(self, desc: UFieldDesc, centres, radius, radius_voxels, factor) -> None:
        """S stamps (reduce_uncertainty_around_position) in one launch, in index order: centres (S, 3), radius (S,), radius_voxels int32 (S,) =
        int(radius / resolution) in the caller's float64, factor (S,)."""
        S = centres.shape[0]
        self._f64(centres, (S, 3), "centres")
        self._f64(radius, (S,), "radius")
        self._f64(factor, (S,), "factor")
        self._i32(radius_voxels, S, "radius_voxels")
        self.lib.ufield("stamp", desc, self.be.ptr(centres), self.be.ptr(radius), self.be.ptr(radius_voxels), self.be.ptr(factor), S, self.be.stream())

    def ufield_update_points(self, desc: UFieldDesc, positions, uncertainties, weights=None, alpha: float = 0.1, workspace=None) -> None:
        """update_uncertainty_field: positions (N, 3), uncertainties (N,), weights (N,) or None; same-voxel points in input order."""
        N = positions.shape[0]
        self._f64(positions, (N, 3), "positions")
        self._f64(uncertainties, (N,), "uncertainties")
        if weights is not None:
            self._f64(weights, (N,), "weights")
        if workspace is None:
            workspace = self.ufield_workspace(tuple(desc.n), 1)
        self._i32(workspace, 0, "workspace")
        keys = self.be.empty((max(N, 1),), "i32")
        self.lib.ufield("update_points", desc, self.be.ptr(positions), self.be.ptr(uncertainties), self.be.ptr(weights), N, float(alpha),
                        self.be.ptr(keys), self.be.ptr(workspace), workspace.shape[0], self.be.stream())

    def ufield_query(self, desc: UFieldDesc, positions):
        """get_uncertainty_at_position for positions (B, 3) -> (B,), 1.0 outside the bounds."""
        B = positions.shape[0]
        self._f64(positions, (B, 3), "positions")
        out = self.be.empty((B,), "f64")
        self.lib.ufield("query", desc, self.be.ptr(positions), B, self.be.ptr(out), self.be.stream())
        return out

    def ufield_statistics(self, desc: UFieldDesc, threshold: float, workspace=None):
        """dict(counts int32 (2,) = observed voxels, voxels above the threshold; values (3,) = sum, min, max of the uncertainty)."""
        if workspace is None:
            workspace = self.ufield_workspace(tuple(desc.n), 1)
        self._i32(workspace, 0, "workspace")
        out = dict(counts=self.be.empty((2,), "i32"), values=self.be.empty((3,), "f64"))
        self.lib.ufield("statistics", desc, float(threshold), self.be.ptr(out["counts"]), self.be.ptr(out["values"]), self.be.ptr(workspace),
                        workspace.shape[0], self.be.stream())
        return out

    def ufield_regions(self, desc: UFieldDesc, threshold: float, min_volume: float, max_regions: int, workspace=None, labels=None):
        """identify_high_uncertainty_regions: dict(labels int32 (n0, n1, n2), regions (max_regions, 12), roots int32 (max_regions,), counts int32
        (2,) = rows written, regions that qualify).  Rows beyond counts[0] are not written."""
        n = tuple(desc.n)
        if workspace is None:
            workspace = self.ufield_workspace(n, max_regions)
        self._i32(workspace, 0, "workspace")
        if labels is None:
            labels = self.be.empty(n, "i32")
        self.be.check(labels, "labels")
        if tuple(labels.shape) != n:
            raise ValueError(f"labels: expected int32 {n}, got {tuple(labels.shape)}")
        rows = max(int(max_regions), 1)
        out = dict(labels=labels, regions=self.be.empty((rows, 12), "f64"), roots=self.be.empty((rows,), "i32"), counts=self.be.empty((2,), "i32"))
        self.lib.ufield("regions", desc, float(threshold), float(min_volume), int(max_regions), self.be.ptr(labels), self.be.ptr(out["regions"]),
                        self.be.ptr(out["roots"]), self.be.ptr(out["counts"]), self.be.ptr(workspace), workspace.shape[0], self.be.stream())
        return out

    def ufield_targets(self, regions, counts, num_targets: int, position=None):
        """The target list of get_exploration_targets from the rows and counts of ufield_regions: (targets (num_targets, 3), n int32 (1,))."""
        self.be.check(regions, "regions")
        self.be.check(counts, "counts")
        targets = self.be.empty((max(int(num_targets), 1), 3), "f64")
        n_out = self.be.empty((1,), "i32")
        self.lib.ufield_targets(self.be.ptr(regions), self.be.ptr(counts), int(num_targets), position, self.be.ptr(targets), self.be.ptr(n_out),
                                self.be.stream())
        return targets, n_out

    # ------------------------------------------------------------------ mission layer: the goal source
    def mission_state(self, B: int):
        """Fresh mission records for B drones (GlobalMissionPlanner.__init__: TAKEOFF, waypoint 0, no global plan yet): float64 (B, 4)."""
        st = self.be.empty((B, MISSION_STATE_WORDS), "f64")
        self.lib.mission_reset(B, self.be.ptr(st), self.be.stream())
        return st

    def _mission_record(self, state, B):
        self.be.check(state, "mission state")
        if tuple(state.shape) != (B, MISSION_STATE_WORDS) or self.be.suffix(state) != "f64":
            raise ValueError(f"mission state: float64 ({B}, {MISSION_STATE_WORDS})")

    def _waypoints(self, waypoints, labels, B) -> list:
        """A waypoint table: positions float64 (W, 3) shared by all drones or (B, W, 3) per drone, labels int32 (W,) or (B, W) -> the five
        table arguments (waypoints, wp_stride, labels, label_stride, W)."""
        self.be.check(waypoints, "waypoints")
        self.be.check(labels, "labels")
        if self.be.suffix(waypoints) != "f64" or waypoints.ndim not in (2, 3) or waypoints.shape[-1] != 3 or (waypoints.ndim == 3 and waypoints.shape[0] != B):
            raise ValueError(f"waypoints: float64 (W, 3) or ({B}, W, 3), got {tuple(waypoints.shape)}")
        W = waypoints.shape[-2]
        if not str(labels.dtype).endswith("int32") or tuple(labels.shape) not in ((W,), (B, W)):
            raise ValueError(f"labels: int32 ({W},) or ({B}, {W}), got {labels.dtype} {tuple(labels.shape)}")
        return [self.be.ptr(waypoints if W else None), 3 * W if waypoints.ndim == 3 else 0, self.be.ptr(labels if W else None), W if labels.ndim == 2 else 0, W]

    def mission_stamps(self, rows: int):
        """An empty stamp table of `rows` rows in the operand form of :meth:`ufield_stamp`: dict(centres (rows, 3), radius (rows,),
        radius_voxels int32 (rows,), factor (rows,))."""
        return dict(centres=self.be.empty((rows, 3), "f64"), radius=self.be.empty((rows,), "f64"), radius_voxels=self.be.empty((rows,), "i32"),
                    factor=self.be.empty((rows,), "f64"))

    def _stamps(self, stamps, rows):
        self._f64(stamps["centres"], (rows, 3), "stamp centres")
        self._f64(stamps["radius"], (rows,), "stamp radius")
        self._f64(stamps["factor"], (rows,), "stamp factor")
        if tuple(self._i32(stamps["radius_voxels"], rows, "stamp radius_voxels").shape) != (rows,):
            raise ValueError(f"stamp radius_voxels: int32 ({rows},)")
        return [self.be.ptr(stamps[k]) for k in ("centres", "radius", "radius_voxels", "factor")]

    def mission_goal(self, mp: MissionParams, state, now, pos, waypoints, labels, resolution: float = 1.0, goal=None, stamps=None):
        """se3mpc_mission_goal_*: GlobalMissionPlanner.get_current_goal for B drones.  state: the mission records (B, 4), updated in place; now:
        float64 (B,), the wall clock of the call; pos (B, 3) float32 or float64; waypoints, labels: the table (:meth:`_waypoints`); resolution: of
        the field the stamps are meant for.  goal, stamps: outputs of an earlier call to be written again.
        -> dict(goal (B, 3) of pos's dtype, stamps = the B-row table :meth:`ufield_stamp` takes: radius_voxels -1 where nothing was stamped)."""
        B = pos.shape[0]
        suf = self.be.suffix(pos)
        self._rows3(pos, B, "pos", suf)
        self._clock(now, B)
        self._mission_record(state, B)
        table = self._waypoints(waypoints, labels, B)
        goal = self.be.empty((B, 3), suf) if goal is None else self._rows3(goal, B, "goal", suf)
        stamps = self.mission_stamps(B) if stamps is None else stamps
        self.lib.loop_call("mission_goal", suf, mp, B, self.be.ptr(now), self.be.ptr(pos), self.be.ptr(state), *table, float(resolution), self.be.ptr(goal),
                           *self._stamps(stamps, B), self.be.stream())
        return dict(goal=goal, stamps=stamps)

    def monte_carlo_mission(self, params: Params, cp: ControllerParams, sp: SimulatorParams, mp: MissionParams, state, mission_state, time, pos, vel,
                            att, omega, waypoints, labels, cycles: int, substeps: int, sim_dt: float, epoch: float = 1000.0, resolution: float = 1.0,
                            wind=None, first_cycle: int = 0, goal=None, want_stamps: bool = False, want_last_plan: bool = False):
        """se3mpc_monte_carlo_mission_*: `cycles` x (mission goal at now = the drone's clock + epoch, solve towards it, `substeps` control + simulator
        steps) for B drones in ONE launch, in place on (state, mission_state, time, pos, vel, att, omega).  The plan's stamps count from
        `first_cycle`: a second call with first_cycle = the cycles already flown continues a run on the same operands.
        -> dict(overflowed as :meth:`monte_carlo`, goal (B, 3) = the last cycle's, stamps = the (cycles * B)-row log of the global plans' stamps
        in the chain's order if `want_stamps` else None, x, accelerations, info of the last cycle's plan if asked for)."""
        B = pos.shape[0]
        suf = self.be.suffix(pos)
        self._drone_state(B, suf, pos, vel, att, omega)
        self._ctrl_state(state, B)
        self._mission_record(mission_state, B)
        self._clock(time, B, "time")
        w_stride = self._wind(wind, B, suf)
        table = self._waypoints(waypoints, labels, B)
        if goal is None:
            goal = self.be.empty((B, 3), suf)
            goal[...] = 0
        self._rows3(goal, B, "goal", suf)
        N = params.horizon
        rows = max(int(cycles), 0) * B
        stamps = self.mission_stamps(rows) if want_stamps else None
        over = self.be.empty((1,), "i32")
        X = self.be.empty((B, 9 * N), suf) if want_last_plan else None
        acc = self.be.empty((B, N, 3), suf) if want_last_plan else None
        info = self.be.empty((B * INFO_DTYPE.itemsize,), "u8") if want_last_plan else None
        self.lib.loop_call("monte_carlo_mission", suf, params, cp, sp, mp, B, int(cycles), int(substeps), float(sim_dt), int(first_cycle), float(epoch), *table,
                           float(resolution), self.be.ptr(wind), w_stride, self.be.ptr(time), self.be.ptr(pos), self.be.ptr(vel), self.be.ptr(att),
                           self.be.ptr(omega), self.be.ptr(state), self.be.ptr(mission_state), self.be.ptr(goal),
                           *(self._stamps(stamps, rows) if want_stamps else [0, 0, 0, 0]), self.be.ptr(X), self.be.ptr(acc), self.be.ptr(info),
                           self.be.ptr(over), self.be.stream())
        return dict(overflowed=over, goal=goal, stamps=stamps, x=X, accelerations=acc, info=info)

    # ------------------------------------------------------------------ problem layout
    def solve(self, params: Params, p0, v0, goal, x0=None, want_trajectory=True, out=None):
        """a7 (+a3, a4, a11, a12): batched L-BFGS-B solve, one wavefront per problem.
        p0, v0, goal: (B, 3);  x0: (B, 9N) or None (reference cold start).  want_trajectory: True (all outputs), False (x and info only:
        restart sweeps) or "accelerations" (x, info, accelerations: the kernel skips attitudes / rates / thrust magnitudes).
        out: a dict this method returned for the same shapes and output set -- its tensors are overwritten and returned (steady-state use).
        -> dict(x (B,9N), info (device bytes), acc/att/rates (B,N,3), thrust (B,N))."""
        N = params.horizon
        for a, nm in ((p0, "p0"), (v0, "v0")) + (((goal, "goal"),) if params.has_goal else ()):
            self.be.check(a, nm)
            if a.ndim != 2 or a.shape[1] != 3 or a.shape[0] != p0.shape[0]:
                raise ValueError(f"{nm}: expected (B, 3), got {tuple(a.shape)}")
        suf = self.be.suffix(p0)
        B = p0.shape[0]
        if x0 is not None:
            self.be.check(x0, "x0")
            if tuple(x0.shape) != (B, 9 * N) or self.be.suffix(x0) != suf:
                raise ValueError(f"x0: expected ({B}, {9 * N}) {suf}")
        if out is not None:
            # steady state: the dict a previous call with the same shapes returned is written again (no allocations)
            X, info, acc, att, rates, thrust = (out[k] for k in ("x", "info", "accelerations", "attitudes", "body_rates", "thrusts"))
            if tuple(X.shape) != (B, 9 * N) or self.be.suffix(X) != suf or info.shape[0] != B * INFO_DTYPE.itemsize:
                raise ValueError(f"out: buffers of another solve shape (expected x ({B}, {9 * N}) {suf})")
            if (acc is None) != (not want_trajectory) or (att is None) != (want_trajectory is not True):
                raise ValueError("out: buffers of another output set (want_trajectory)")
        else:
            X = self.be.empty((B, 9 * N), suf)
            info = self.be.empty((B * INFO_DTYPE.itemsize,), "u8")
            acc = att = rates = thrust = None
            if want_trajectory == "accelerations":            # what a closed loop reading the plan in place needs next to x (se3mpc_closed_loop_*)
                acc = self.be.empty((B, N, 3), suf)
            elif want_trajectory:
                acc, att, rates = (self.be.empty((B, N, 3), suf) for _ in range(3))
                thrust = self.be.empty((B, N), suf)
        self.lib.call("solve", suf, B, self.be.ptr(p0), self.be.ptr(v0), self.be.ptr(goal if params.has_goal else None),
                      self.be.ptr(x0), self.be.ptr(X), self.be.ptr(info), self.be.ptr(acc), self.be.ptr(att),
                      self.be.ptr(rates), self.be.ptr(thrust), self.be.stream(), params=params)
        return dict(x=X, info=info, accelerations=acc, attitudes=att, body_rates=rates, thrusts=thrust)

    def solve_packed(self, params: Params, inputs, x0=None, out=None, host_mapped=False, stream=None):
        """Latency-oriented form of :meth:`solve` for the planner: ONE device buffer in, ONE out.
        inputs: (3, B, 3) = stacked (p0, v0, goal) [goal ignored when has_goal == 0];
        out: uint8 buffer of :meth:`packed_size` bytes (allocated if None) laid out as
        [X | acc | att | rates | thrust | info]; decode on the host with :meth:`unpack_solution`.
        host_mapped=True: `inputs`, `x0` and `out` are PINNED host tensors; the kernel reads and writes them in
        place over the host link (hipHostMalloc memory is mapped into the device's address space under the
        same address), which for a handful of problems beats two staged copies.  The caller synchronises the
        stream before reading `out`."""
        N = params.horizon
        if host_mapped:
            for name, a in (("inputs", inputs), ("x0", x0), ("out", out)):
                if a is None and name == "x0":
                    continue
                if a is None or not self.be.is_host_mapped(a):
                    raise TypeError(f"{name}: host_mapped=True needs a pinned, contiguous host tensor")
        else:
            self.be.check(inputs, "inputs")
        if inputs.ndim != 3 or inputs.shape[0] != 3 or inputs.shape[2] != 3:
            raise ValueError(f"inputs: expected (3, B, 3), got {tuple(inputs.shape)}")
        suf = self.be.suffix(inputs)
        B = inputs.shape[1]
        esz = 4 if suf == "f32" else 8
        if out is None:
            out = self.be.empty((self.packed_size(B, N, suf),), "u8")
        base = self.be.ptr(out)
        o_x, o_acc, o_att, o_rates, o_thr, o_info, _ = self._packed_offsets(B, N, esz)
        step = B * 3 * esz
        pin = self.be.ptr(inputs)
        self.lib.call("solve", suf, B, pin, pin + step, (pin + 2 * step) if params.has_goal else 0, self.be.ptr(x0),
                      base + o_x, base + o_info, base + o_acc, base + o_att, base + o_rates, base + o_thr,
                      self.be.stream() if stream is None else stream, params=params)
        return out

    @staticmethod
    def _packed_offsets(B, N, esz):
        o_x = 0
        o_acc = o_x + B * 9 * N * esz
        o_att = o_acc + B * 3 * N * esz
        o_rates = o_att + B * 3 * N * esz
        o_thr = o_rates + B * 3 * N * esz
        o_info = (o_thr + B * N * esz + 7) // 8 * 8
        return o_x, o_acc, o_att, o_rates, o_thr, o_info, o_info + B * INFO_DTYPE.itemsize

    def packed_size(self, B, N, suffix) -> int:
        return self._packed_offsets(B, N, 4 if suffix == "f32" else 8)[-1]

    def unpack_solution(self, host_bytes: np.ndarray, B: int, N: int, suffix: str):
        """Decode a packed result into float64 arrays that do not alias `host_bytes` (which the caller reuses):
        f64 = ONE copy of the buffer and views into it, f32 = one widening cast per field."""
        esz, dt = (4, np.float32) if suffix == "f32" else (8, np.float64)
        o_x, o_acc, o_att, o_rates, o_thr, o_info, end = self._packed_offsets(B, N, esz)
        raw = host_bytes[:end].copy()
        # the five float fields are one contiguous run: ONE view (f64) or ONE widening cast (f32), then slices of it
        nfl = (o_thr + B * N * esz) // esz
        allf = np.frombuffer(raw, dtype=dt, count=nfl)
        if esz == 4:
            allf = allf.astype(np.float64)
        f = lambda lo, cnt, shape: allf[lo // esz:lo // esz + cnt].reshape(shape)
        return dict(x=f(o_x, B * 9 * N, (B, 9 * N)), accelerations=f(o_acc, B * 3 * N, (B, N, 3)),
                    attitudes=f(o_att, B * 3 * N, (B, N, 3)), body_rates=f(o_rates, B * 3 * N, (B, N, 3)),
                    thrusts=f(o_thr, B * N, (B, N)), info=np.frombuffer(raw, dtype=INFO_DTYPE, count=B, offset=o_info))

    def info_to_host(self, info) -> np.ndarray:
        """Device bytes of se3mpc_solve_info[B] -> NumPy structured array (synchronises)."""
        return np.frombuffer(self.be.to_host(info).tobytes(), dtype=INFO_DTYPE)
