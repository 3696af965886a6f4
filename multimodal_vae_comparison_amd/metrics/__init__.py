"""The forward-only evaluation metrics, one module per kernel file of csrc/.  Callers use them through `ops` (ops.py imports
every public name); the argument checks they share are in _checks.py."""
