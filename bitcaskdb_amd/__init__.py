"""bitcaskdb_amd: MI355X-native WAL record codec for bitcaskDB's compaction / recovery scan.

The product is libbcw.so (C-ABI in include/bcw.h, HIP kernels for gfx950 in csrc/). This package
is the Python host mirror of the reference interface (wal.py: the WAL iterators, compaction re-encode,
hint rebuild; index.py: the device-resident index, its rebuild from hint / data WALs, the device
compaction filter and the batched Get by key against resident WALs; write.py: the batched Write into the
active WAL's resident image; usage.py: live and freed bytes per WAL file for the compaction picker; scrub.py: every
index entry verified against the resident WALs; scan.py: the index listed and folded by key prefix) and its ctypes
binding (_lib.py).
"""
from . import _lib
from .wal import (Context, Decoded, ErrCorruptedHintRecord, ErrInvalidData, ErrShortFile, ErrWalMismatchBlockSize,
                  ErrWalMismatchCRC, ErrWalMismatchMagic, ErrWalUnknownRecordType, HintRecord, Meta, Record,
                  RefPanic, Wal, WalError, WalFile, compact_one_wal, compute_crc32, default_context, iterate_hint,
                  iterate_record, load_wal, new_hint_by_wal)
from .staging import Stage
from .index import (ErrKeyNotFound, ErrKeySoftDeleted, GetBatch, Index, WalSet, compact_one_wal_filtered, merged_key,
                    murmur3_sum64, recover_from_wals)
from .write import ActiveWal, WriteBatch
from .usage import FidUsage, FidUsageMap, PickerWalInfo, default_compaction_picker, drop_fids, wal_garbage
from .scrub import BadEntry, ScrubReport, verify_index
from .scan import ScanGroup, ScanReport, fold_index, scan_index

__all__ = ["Context", "Decoded", "ErrCorruptedHintRecord", "ErrInvalidData", "ErrShortFile",
           "ErrWalMismatchBlockSize", "ErrWalMismatchCRC", "ErrWalMismatchMagic", "ErrWalUnknownRecordType",
           "HintRecord", "Meta", "Record", "RefPanic", "Wal", "WalError", "compute_crc32", "default_context",
           "iterate_hint", "iterate_record", "load_wal", "_lib", "WalFile", "compact_one_wal",
           "new_hint_by_wal", "ErrKeyNotFound", "ErrKeySoftDeleted", "Index", "compact_one_wal_filtered",
           "merged_key", "murmur3_sum64", "recover_from_wals", "Stage", "WalSet", "GetBatch", "ActiveWal",
           "WriteBatch", "FidUsage", "PickerWalInfo", "default_compaction_picker", "wal_garbage",
           "FidUsageMap", "drop_fids", "BadEntry", "ScrubReport", "verify_index", "ScanGroup", "ScanReport", "scan_index",
           "fold_index"]
