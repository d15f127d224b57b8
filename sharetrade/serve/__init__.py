"""Policy serving: batched ``SelectionAction`` inference on the GPU (``csrc/qserve.hip``).

* :class:`PolicyServer` — resident weights, one launch per request batch, hot weight swaps;
* :class:`DynamicBatcher` — single requests from many client threads -> server batches;
* :class:`PolicyServingActor` — the reference's actor message API over the server;
* :meth:`PolicyServer.backtest` — whole episodes of a frozen policy in one launch (``csrc/qrollout.hip``,
  :class:`RolloutKernel`, oracle :func:`reference_rollout`), with the on-chip risk ledger (:class:`QLedger`,
  oracle ``rollout.ledger_from_trace``) behind ``BacktestResult.report()``;
* :class:`GruPolicy` — a frozen GRU(256) policy of config 5 and its backtest on minute bars
  (``csrc/gru_rollout.hip``, oracle :func:`reference_gru_rollout`), with the on-chip risk ledger
  (:class:`GruLedger`, oracle :func:`ledger_from_trace`) behind ``GruBacktestResult.report()``;
* :class:`GruSessionServer` / :class:`GruBatcher` — serving that policy: stateful sessions, one bar per launch
  (``csrc/gru_serve.hip``, oracle :func:`reference_gru_serve`).
"""
from .actor import LoadPolicy, PolicyLoaded, PolicyServingActor
from .gru_rollout import (GruBacktestResult, GruLedger, GruPolicy, ledger_from_trace, reference_gru_rollout,
                          simulate_minute_actions)
from .gru_serve import GruBatcher, GruDecision, GruSessionServer, reference_gru_serve
from .kernel import ServeKernel, reference_select, supported
from .rollout import BacktestResult, QLedger, RolloutKernel, RolloutParams, reference_rollout
from .server import DynamicBatcher, PolicyServer

__all__ = ["PolicyServer", "DynamicBatcher", "PolicyServingActor", "LoadPolicy", "PolicyLoaded", "ServeKernel",
           "reference_select", "supported", "BacktestResult", "QLedger", "RolloutKernel", "RolloutParams", "reference_rollout",
           "GruPolicy", "GruBacktestResult", "GruLedger", "ledger_from_trace", "reference_gru_rollout",
           "simulate_minute_actions",
           "GruSessionServer", "GruBatcher", "GruDecision", "reference_gru_serve"]
