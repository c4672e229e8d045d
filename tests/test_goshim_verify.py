"""The Go shim's verification state (no Go toolchain here, so the sources are checked as text, CPU only): the marker that a C handle has
received its G2 points is keyed by the C handle, guarded by the handle map's mutex and cleared where the handle is freed, so a settings
object used again after CloseHip (or a new object at a reused address) hands its G2 points to the new handle."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "go-kzg_amd", "goshim")


def src(*parts):
    return re.sub(r"//[^\n]*", "", open(os.path.join(SHIM, *parts)).read())


def func_body(text, signature):
    i = text.index(signature)
    depth, j = 0, text.index("{", i)
    for k in range(j, len(text)):
        depth += {"{": 1, "}": -1}.get(text[k], 0)
        if depth == 0:
            return text[j:k + 1]
    raise AssertionError(signature)


def test_kzg_secret_g2_marker_follows_the_c_handle():
    v = src("kzg", "verify_hip.go")
    assert "sync.Map" not in v
    body = func_body(v, "func (ks *KZGSettings) hipSecretG2()")
    assert "hipMu.Lock()" in body and "hipSecretG2Set[key] != h" in body and "hipSecretG2Set[key] = h" in body
    assert body.index("hipMu.Lock()") < body.index("C.kzg_hip_kzg_set_secret_g2(")
    close = func_body(src("kzg", "hip_binding.go"), "func (ks *KZGSettings) CloseHip()")
    assert "delete(hipSecretG2Set, uintptr(unsafe.Pointer(ks)))" in close
    assert close.index("delete(hipSecretG2Set") < close.index("C.kzg_hip_kzg_settings_free(")
    for name in ("CheckProofSingleBatch", "CheckProofMultiBatch"):
        assert "ks.hipSecretG2()" in func_body(v, "func (ks *KZGSettings) %s(" % name)


def test_eth_setup_g2_marker_follows_the_c_handle():
    v = src("eth", "verify_hip.go")
    assert "sync.Once" not in v
    body = func_body(v, "func VerifyKZGProofBatch(")
    assert "hipSetupG2Mu.Lock()" in body and "hipSetupG2For != hipEth" in body and "hipSetupG2For = hipEth" in body
    close = func_body(src("eth", "eth_hip.go"), "func CloseHip()")
    assert "hipSetupG2For = nil" in close and close.index("hipSetupG2For = nil") < close.index("C.kzg_hip_eth_settings_free(")
    # invalid rows take the reference's own error texts (VerifyKZGProof on the CPU names the input and the cause)
    assert "VerifyKZGProof(commitments[i], zs[i], ys[i], proofs[i])" in body
