"""CPU: the verified exchange in the C ABI -- mumemto_gpu.h declares mmt_comm_verify_stats and mmt_exchange_digest, the
library exports them, and the ABI version says so (7)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mmt_comm_verify_stats", "mmt_exchange_digest")


def test_header_declares_the_verification_entry_points():
    src = open(os.path.join(ROOT, "include", "mumemto_gpu.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW:
        assert re.search(r"MMT_API\s+int\s+%s\s*\(" % name, src), name
    assert re.search(r"mmt_comm_verify_stats\s*\(\s*mmt_comm\s*\*\s*\w*\s*,\s*uint64_t\s+\w+\[8\]\s*\)", src)
    assert re.search(r"mmt_exchange_digest\s*\(\s*const\s+void\s*\*\s*\w+\s*,\s*uint64_t\s+\w+\s*,\s*uint32_t\s+\w+\s*,\s*uint64_t\s+\w+\s*,"
                     r"\s*uint64_t\s*\*\s*\w+\s*\)", src)


def test_library_exports_them_and_the_abi_version_is_7():
    import mumemto_amd
    from mumemto_amd import binding, build
    build.build()
    L = mumemto_amd.load_library()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in binding.GPU_ABI_SYMBOLS
    assert L.mmt_abi_version() == 7
    assert callable(mumemto_amd.exchange_digest) and hasattr(mumemto_amd.Comm, "verify_stats")
