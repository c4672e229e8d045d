//go:build kzg_hip && !bignum_pure && !bignum_hol256 && !bignum_hbls
// +build kzg_hip,!bignum_pure,!bignum_hol256,!bignum_hbls

// eth.VerifyKZGProofBatch: eth.VerifyKZGProof (eth/eth.go:114-135) over many proofs in one device call.  A lone VerifyKZGProof (and through
// it PointEvaluationPrecompile, VerifyAggregateKZGProof, ValidateBlobsSidecar) stays on Kilic (INTEGRATION.md).
package eth

/*
#cgo LDFLAGS: -lkzg_hip
#include "kzg_hip.h"
*/
import "C"

import (
	"sync"
	"unsafe"
)

// the eth handle that has received kzgSetupG2 (kzg_hip_eth_set_setup_g2); CloseHip (eth_hip.go) clears it with the handle
var (
	hipSetupG2Mu  sync.Mutex
	hipSetupG2For *C.kzg_hip_eth
)

// VerifyKZGProofBatch: (ok[i], errs[i]) = VerifyKZGProof(commitments[i], zs[i], ys[i], proofs[i]), with the reference's error texts.
func VerifyKZGProofBatch(commitments []KZGCommitment, zs, ys [][32]byte, proofs []KZGProof) ([]bool, []error) {
	n := len(commitments)
	if len(zs) != n || len(ys) != n || len(proofs) != n {
		panic("VerifyKZGProofBatch: slices of different lengths")
	}
	oks, errs := make([]bool, n), make([]error, n)
	if n == 0 {
		return oks, errs
	}
	hipSetupG2Mu.Lock()
	if hipSetupG2For != hipEth {
		if st := C.kzg_hip_eth_set_setup_g2(hipEth, unsafe.Pointer(&kzgSetupG2[0]), C.uint64_t(len(kzgSetupG2))); st != C.KZG_HIP_OK {
			hipSetupG2Mu.Unlock()
			panic("kzg_hip: eth_set_setup_g2 failed")
		}
		hipSetupG2For = hipEth
	}
	hipSetupG2Mu.Unlock()
	res := make([]uint8, n)
	if st := C.kzg_hip_eth_verify_kzg_proof_batch(hipEth, unsafe.Pointer(&commitments[0]), unsafe.Pointer(&zs[0]), unsafe.Pointer(&ys[0]),
		unsafe.Pointer(&proofs[0]), C.uint64_t(n), (*C.uint8_t)(unsafe.Pointer(&res[0]))); st != C.KZG_HIP_OK {
		panic("kzg_hip: eth_verify_kzg_proof_batch failed")
	}
	for i, r := range res {
		switch r {
		case 1:
			oks[i] = true
		case 2, 3:
			// invalid inputs (the cold path): the reference's own parsing on the CPU names the input and the cause, with its error texts
			_, errs[i] = VerifyKZGProof(commitments[i], zs[i], ys[i], proofs[i])
			if errs[i] == nil {
				panic("kzg_hip: eth_verify_kzg_proof_batch rejected inputs that VerifyKZGProof accepts")
			}
		}
	}
	return oks, errs
}
