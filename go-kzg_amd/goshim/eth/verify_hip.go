//go:build kzg_hip && !bignum_pure && !bignum_hol256 && !bignum_hbls
// +build kzg_hip,!bignum_pure,!bignum_hol256,!bignum_hbls

// eth.VerifyKZGProofBatch: eth.VerifyKZGProof (eth/eth.go:114-135) over many proofs in one device call, and VerifyAggregateKZGProofBatch /
// ValidateBlobsSidecarBatch: the block-level verifier (eth/eth.go:155-208) over many sidecars in one device call.  A lone VerifyKZGProof, a lone
// PointEvaluationPrecompile and the pairing of a lone VerifyAggregateKZGProof / ValidateBlobsSidecar stay on Kilic (INTEGRATION.md); batches of
// precompile inputs are served by PointEvaluationPrecompileBatch (exec_hip.go).
package eth

/*
#cgo LDFLAGS: -lkzg_hip
#include "kzg_hip.h"
*/
import "C"

import (
	"errors"
	"fmt"
	"sync"
	"unsafe"

	"github.com/protolambda/go-kzg/bls"
)

// the eth handle that has received kzgSetupG2 (kzg_hip_eth_set_setup_g2); CloseHip (eth_hip.go) clears it with the handle.
// hipEnsureSetupG2 (exec_hip.go) is the lock / set / mark step as a function; the two copies of it below predate it and do the same:
// a change to that step belongs in all three places (or replaces the two copies by calls of the helper).
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

// VerifyKZGProofBatchCombined: what VerifyKZGProofBatch returns, with one pairing check per group of rows (a random linear combination per group; rows
// with invalid inputs drop out of it, the rows of a failing group are re-checked one by one).  seed: nil draws the weights' seed from the operating
// system; 32 bytes make a run reproducible -- a seed the prover can know in advance voids the 2^-128 bound.
func VerifyKZGProofBatchCombined(commitments []KZGCommitment, zs, ys [][32]byte, proofs []KZGProof, seed *[32]byte) ([]bool, []error) {
	n := len(commitments)
	if len(zs) != n || len(ys) != n || len(proofs) != n {
		panic("VerifyKZGProofBatchCombined: slices of different lengths")
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
	var sp *C.uint8_t
	if seed != nil {
		sp = (*C.uint8_t)(unsafe.Pointer(&seed[0]))
	}
	res := make([]uint8, n)
	if st := C.kzg_hip_eth_verify_kzg_proof_batch_combined(hipEth, unsafe.Pointer(&commitments[0]), unsafe.Pointer(&zs[0]), unsafe.Pointer(&ys[0]),
		unsafe.Pointer(&proofs[0]), C.uint64_t(n), sp, (*C.uint8_t)(unsafe.Pointer(&res[0]))); st != C.KZG_HIP_OK {
		panic("kzg_hip: eth_verify_kzg_proof_batch_combined failed")
	}
	for i, r := range res {
		switch r {
		case 1:
			oks[i] = true
		case 2, 3:
			// invalid inputs (the cold path): the reference's own parsing on the CPU names the input and the cause, with its error texts
			_, errs[i] = VerifyKZGProof(commitments[i], zs[i], ys[i], proofs[i])
			if errs[i] == nil {
				panic("kzg_hip: eth_verify_kzg_proof_batch_combined rejected inputs that VerifyKZGProof accepts")
			}
		}
	}
	return oks, errs
}

// VerifyAggregateKZGProofBatch: (ok[j], errs[j]) = VerifyAggregateKZGProof(blobs[j], expectedKZGCommitments[j], proofs[j]) (eth/eth.go:155-172)
// for many blocks in one device call: transcripts, aggregation, evaluation and the pairing all run there.  A block without blobs is valid input.
func VerifyAggregateKZGProofBatch(blobs []BlobSequence, expectedKZGCommitments []KZGCommitmentSequence, proofs []KZGProof) ([]bool, []error) {
	s := len(blobs)
	if len(expectedKZGCommitments) != s || len(proofs) != s {
		panic("VerifyAggregateKZGProofBatch: slices of different lengths")
	}
	oks, errs := make([]bool, s), make([]error, s)
	if s == 0 {
		return oks, errs
	}
	counts := make([]uint64, s)
	total := 0
	for j := range blobs {
		if expectedKZGCommitments[j].Len() != blobs[j].Len() {
			panic("got LinCombG1 numbers/factors length mismatch") // what the reference does here: bls.LinCombG1's panic (eth/helpers.go:159)
		}
		counts[j] = uint64(blobs[j].Len())
		total += blobs[j].Len()
	}
	flat := make([]Blob, total)
	comms := make([]KZGCommitment, total)
	at := 0
	for j := range blobs {
		for i := 0; i < blobs[j].Len(); i++ {
			flat[at] = blobs[j].At(i)
			comms[at] = expectedKZGCommitments[j].At(i)
			at++
		}
	}
	var bp, cp unsafe.Pointer
	if total > 0 {
		bp, cp = unsafe.Pointer(&flat[0]), unsafe.Pointer(&comms[0])
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
	res := make([]uint8, s)
	if st := C.kzg_hip_eth_verify_aggregate_kzg_proof_batch(hipEth, bp, (*C.uint64_t)(unsafe.Pointer(&counts[0])), cp, unsafe.Pointer(&proofs[0]),
		C.uint64_t(s), (*C.uint8_t)(unsafe.Pointer(&res[0])), nil, nil, nil); st != C.KZG_HIP_OK {
		panic(fmt.Sprintf("kzg_hip: eth_verify_aggregate_kzg_proof_batch: status %d", int(st)))
	}
	for j, r := range res {
		switch r {
		case 1:
			oks[j] = true
		case 2:
			errs[j] = errors.New("could not convert blobs to polynomials")
		case 3:
			// invalid encodings (the cold path): the reference's own parsing on the CPU names the input, in its order (eth/helpers.go:153-156, eth/eth.go:166-169)
			for i := 0; i < expectedKZGCommitments[j].Len() && errs[j] == nil; i++ {
				c := expectedKZGCommitments[j].At(i)
				_, errs[j] = bls.FromCompressedG1(c[:])
			}
			if errs[j] == nil {
				if _, err := bls.FromCompressedG1(proofs[j][:]); err != nil {
					errs[j] = fmt.Errorf("failed to decode kzgProof: %v", err)
				}
			}
			if errs[j] == nil {
				panic("kzg_hip: eth_verify_aggregate_kzg_proof_batch rejected inputs that the reference's parsing accepts")
			}
		}
	}
	return oks, errs
}

// ValidateBlobsSidecarBatch: errs[j] = ValidateBlobsSidecar(slots[j], beaconBlockRoots[j], expectedKZGCommitments[j], blobsSidecars[j])
// (eth/eth.go:185-208).  The slot, root and length checks run per row on the host; the rows that pass them share one device call.
func ValidateBlobsSidecarBatch(slots []Slot, beaconBlockRoots []Root, expectedKZGCommitments []KZGCommitmentSequence, blobsSidecars []BlobsSidecar) []error {
	s := len(blobsSidecars)
	if len(slots) != s || len(beaconBlockRoots) != s || len(expectedKZGCommitments) != s {
		panic("ValidateBlobsSidecarBatch: slices of different lengths")
	}
	errs := make([]error, s)
	var rows []int
	var blobs []BlobSequence
	var comms []KZGCommitmentSequence
	var proofs []KZGProof
	for j, sc := range blobsSidecars {
		switch {
		case slots[j] != sc.BeaconBlockSlot:
			errs[j] = fmt.Errorf("slot doesn't match sidecar's beacon block slot (%v != %v)", slots[j], sc.BeaconBlockSlot)
		case beaconBlockRoots[j] != sc.BeaconBlockRoot:
			errs[j] = errors.New("roots not equal")
		case sc.Blobs.Len() != expectedKZGCommitments[j].Len():
			errs[j] = fmt.Errorf("blob len doesn't match expected kzg commitments len (%v != %v)", sc.Blobs.Len(), expectedKZGCommitments[j].Len())
		default:
			rows = append(rows, j)
			blobs = append(blobs, sc.Blobs)
			comms = append(comms, expectedKZGCommitments[j])
			proofs = append(proofs, sc.KZGAggregatedProof)
		}
	}
	oks, verr := VerifyAggregateKZGProofBatch(blobs, comms, proofs)
	for i, j := range rows {
		if verr[i] != nil {
			errs[j] = fmt.Errorf("verify_aggregate_kzg_proof error: %v", verr[i])
		} else if !oks[i] {
			errs[j] = errInvalidKZGProof
		}
	}
	return errs
}
