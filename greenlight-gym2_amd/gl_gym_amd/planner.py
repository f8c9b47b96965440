"""Sampling-based planning on the device (include/glgym.h glgym_plan_*): from the current state of each of an environment's B
greenhouses, simulate K candidate control sequences over H env-steps on forked copies, score them by their discounted return, and
pick the best per greenhouse (random shooting) or the exponentially weighted mean sequence (MPPI).  The reference has no counterpart;
its README lists MPC as a next step.

What the planner sees: PERFECT-FORECAST MPC.  The children step on the true future rows of the environment's weather table -- the
rows the observation's forecast module exposes -- clamped at the end of the table.  No noise is drawn inside the horizon: with
crop="current" the parent's present crop block is held over the horizon, with "nominal" the handle's parameters are used.  No reset
happens either: a child that reaches its season end stops accumulating (`alive`), the step that reports `done` being its last.

The parent environment is only read: its state, random streams, draw counter, episode counters, metrics() and step_flags_t are after
a rollout what they were before."""
from __future__ import annotations

import ctypes as C
from typing import Any, Dict, Optional

from . import _lib as L


class Planner:
    def __init__(self, env, n_candidates: int, horizon: int, gamma: float = 1.0, crop: str = "nominal"):
        if int(n_candidates) < 1 or int(horizon) < 1:
            raise ValueError("n_candidates and horizon must be at least 1")
        if crop not in ("nominal", "current"):
            raise ValueError("crop must be 'nominal' or 'current'")
        if not (float(gamma) >= 0.0) or float(gamma) == float("inf"):
            raise ValueError("gamma must be finite and >= 0")
        torch = env.torch
        self.env, self.torch = env, torch
        self.K, self.H, self.gamma, self.crop = int(n_candidates), int(horizon), float(gamma), crop
        self.B = env.B
        self.C = self.B * self.K                                     # children
        self.ld = (self.C + 63) // 64 * 64
        dev, T = env.device, env.tdtype
        z = lambda *s, dtype=T: torch.zeros(*s, dtype=dtype, device=dev)  # noqa: E731
        # the children's environment buffers (what glgym_step reads and writes) ...
        self.x_T, self.u_T = z(L.NX, self.ld), z(L.NU, self.ld)
        self.timestep_t, self.w_off_t = z(self.C, dtype=torch.int32), z(self.C, dtype=torch.int32)
        self.start_day_t = z(self.C, dtype=torch.float32)
        self.crop_T = z(L.NCROP, self.ld) if (crop == "current" and env.crop_T is not None) else None
        self.reward_t, self.info_T = z(self.ld), z(L.NINFO, self.ld)
        self.done_t = z(self.C, dtype=torch.uint8)
        self.step_flags_t = z(self.C, dtype=torch.int32)
        # ... their accumulators ...
        self.ret_t = z(self.C, dtype=torch.float64)
        self.viol_T = z(3, self.ld, dtype=torch.float64)
        self.n_steps_t = z(self.C, dtype=torch.int32)
        self.alive_t, self.failed_t = z(self.C, dtype=torch.uint8), z(self.C, dtype=torch.uint8)
        # ... and the selection's outputs
        self.best_k_t = z(self.B, dtype=torch.int32)
        self.best_ret_t = z(self.B, dtype=torch.float64)
        self.best_action_t = z(self.B, L.NU, dtype=torch.float32)
        self.best_sequence_t = z(self.H, self.B, L.NU, dtype=torch.float32)
        self.mean_sequence_t = z(self.H, self.B, L.NU, dtype=torch.float32)
        self._actions_buf = self._controls_T = None                  # staging, allocated at first use
        self._actions = None                                         # the [H, C, 6] block of the last rollout (select reads it)
        self.x, self.u = self.x_T[:, :self.C].t(), self.u_T[:, :self.C].t()

    def set_layout(self, layout: str):
        """Kernel layout of float32 env-steps (TomatoVecEnv.set_layout; handle state, shared with the environment).  With "auto" the
        CHILD batch decides for the planner's steps: four lanes per environment up to 16 384 children, one lane beyond."""
        self.env.set_layout(layout)

    # ------------------------------------------------------------------------------------------------
    def fork(self, parent_t=None):
        """Copy the environment's current state into the children and zero their accumulators (rollout() calls this).  parent_t:
        optional int32 [B*K] parent index per child; default child c <- environment c // K."""
        e = self.env
        if parent_t is not None and (parent_t.dtype != self.torch.int32 or parent_t.numel() != self.C or not parent_t.is_contiguous()):
            raise ValueError(f"parent_t must be a contiguous int32 tensor of {self.C} entries")
        a = L.make_plan_args(L.PlanForkArgs, self.C, e.B, self.K, e.ld, self.ld, parent_t.data_ptr() if parent_t is not None else None,
                             e.x_T.data_ptr(), e.u_T.data_ptr(), e.timestep_t.data_ptr(), e.w_off_t.data_ptr(), e.start_day_t.data_ptr(),
                             e.crop_T.data_ptr() if self.crop_T is not None else None,
                             self.x_T.data_ptr(), self.u_T.data_ptr(), self.timestep_t.data_ptr(), self.w_off_t.data_ptr(),
                             self.start_day_t.data_ptr(), self.crop_T.data_ptr() if self.crop_T is not None else None,
                             self.ret_t.data_ptr(), self.viol_T.data_ptr(), self.n_steps_t.data_ptr(), self.alive_t.data_ptr(),
                             self.failed_t.data_ptr())
        L.check(e._lib.glgym_plan_fork(e._h, C.byref(a), e._stream()), "glgym_plan_fork")

    def _step_args(self):
        e = self.env
        return L.make_step_args(self.C, self.ld, self.x_T.data_ptr(), self.u_T.data_ptr(), None, None, e.weather_t.data_ptr(),
                                e.weather_rows, self.w_off_t.data_ptr(), self.timestep_t.data_ptr(),
                                self.crop_T.data_ptr() if self.crop_T is not None else None, e.N, self.reward_t.data_ptr(),
                                self.info_T.data_ptr(), self.done_t.data_ptr(), None, self.step_flags_t.data_ptr())

    def rollout(self, actions_t=None, controls_t=None):
        """Fork from the environment's current state and run the H-step rollout of every candidate.
        actions_t [H, B*K, 6] (or [H, B, K, 6]) f32 in [-1, 1]: the action path of step_tensor; a contiguous float32 tensor on the
        environment's device is read in place.  controls_t [H, B*K, 6]: raw controls (step_raw_control).  Child b*K + k is candidate k
        of environment b.
        Returns device tensors (views of the planner's buffers, overwritten by the next rollout): returns [B, K] f64, alive [B, K] u8,
        steps [B, K] i32, violations [3, B, K] f64 (co2, temp, rh), failed [B, K] u8."""
        if (actions_t is None) == (controls_t is None):
            raise ValueError("give exactly one of actions_t / controls_t")
        torch, e = self.torch, self.env
        n = self.H * self.C * L.NU
        act_ptr = ctl_ptr = None
        if actions_t is not None:
            if actions_t.numel() != n:
                raise ValueError(f"actions_t must hold horizon x (num_envs * n_candidates) x 6 = {n} values, got {tuple(actions_t.shape)}")
            if actions_t.dtype == torch.float32 and actions_t.is_cuda and actions_t.device == e.device and actions_t.is_contiguous():
                self._actions = actions_t.view(self.H, self.C, L.NU)
            else:
                if self._actions_buf is None:
                    self._actions_buf = torch.zeros(self.H, self.C, L.NU, dtype=torch.float32, device=e.device)
                self._actions_buf.copy_(actions_t.reshape(self.H, self.C, L.NU))
                self._actions = self._actions_buf
            act_ptr = self._actions.data_ptr()
        else:
            if controls_t.numel() != n:
                raise ValueError(f"controls_t must hold horizon x (num_envs * n_candidates) x 6 = {n} values, got {tuple(controls_t.shape)}")
            if self._controls_T is None:
                self._controls_T = torch.zeros(self.H, L.NU, self.ld, dtype=e.tdtype, device=e.device)
            self._controls_T[:, :, :self.C].copy_(controls_t.reshape(self.H, self.C, L.NU).transpose(1, 2))
            self._actions = None
            ctl_ptr = self._controls_T.data_ptr()
        self.fork()
        a = L.make_plan_args(L.PlanRolloutArgs, self.H, self.gamma, self._step_args(), act_ptr, ctl_ptr, self.ret_t.data_ptr(),
                             self.viol_T.data_ptr(), self.n_steps_t.data_ptr(), self.alive_t.data_ptr(), self.failed_t.data_ptr())
        L.check(e._lib.glgym_plan_rollout(e._h, C.byref(a), e._stream()), "glgym_plan_rollout")
        B, K = self.B, self.K
        return (self.ret_t.view(B, K), self.alive_t.view(B, K), self.n_steps_t.view(B, K), self.viol_T[:, :self.C].view(3, B, K),
                self.failed_t.view(B, K))

    def select(self, temperature: Optional[float] = None, sequence: bool = False) -> Dict[str, Any]:
        """Best candidate per environment from the last rollout: {"best_k" [B] i32 (-1: every candidate failed or came back
        non-finite), "best_return" [B] f64 (NaN then), "best_action" [B, 6] f32 = the best candidate's first action (zeros then)}, with
        sequence=True also "best_sequence" [H, B, 6], with temperature > 0 also "mean_sequence" [H, B, 6]: the MPPI mean with weights
        exp((return - max) / temperature) over the admissible candidates.  After a rollout of raw controls only best_k / best_return
        are available.  Device tensors, overwritten by the next call."""
        e = self.env
        has_a = self._actions is not None
        if not has_a and (sequence or temperature is not None):
            raise ValueError("best_sequence / mean_sequence need a rollout of actions_t")
        if temperature is not None and not float(temperature) > 0.0:
            raise ValueError("temperature must be > 0")
        a = L.make_plan_args(L.PlanSelectArgs, self.B, self.K, self.H, self.ret_t.data_ptr(), self.failed_t.data_ptr(),
                             self._actions.data_ptr() if has_a else None, self.best_k_t.data_ptr(), self.best_ret_t.data_ptr(),
                             self.best_action_t.data_ptr() if has_a else None, self.best_sequence_t.data_ptr() if sequence else None,
                             float(temperature) if temperature is not None else 0.0,
                             self.mean_sequence_t.data_ptr() if temperature is not None else None)
        L.check(e._lib.glgym_plan_select(e._h, C.byref(a), e._stream()), "glgym_plan_select")
        out = {"best_k": self.best_k_t, "best_return": self.best_ret_t}
        if has_a:
            out["best_action"] = self.best_action_t
        if sequence:
            out["best_sequence"] = self.best_sequence_t
        if temperature is not None:
            out["mean_sequence"] = self.mean_sequence_t
        return out
