"""Decode engine (on-device arm)."""
from .engine import OLLAMA_DEFAULTS, DecodeEngine, GenResult, ScoreResult, logprob_host  # noqa: F401
