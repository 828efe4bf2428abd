"""josefine_amd — MI355X-native batched Chained-Raft engine (hot path of
tychedelia/josefine's src/raft behind a C ABI)."""
from . import _capi as capi
from .engine import BatchedRaft, Command, DenseCluster, DeviceRows, EngineError, GroupImage, RaftHandle, commit_rows_as_fsm, device_api, expand_fsm_rows, move_groups

__all__ = ["BatchedRaft", "Command", "DenseCluster", "DeviceRows", "EngineError", "GroupImage", "RaftHandle", "capi", "commit_rows_as_fsm", "device_api", "expand_fsm_rows", "move_groups"]
