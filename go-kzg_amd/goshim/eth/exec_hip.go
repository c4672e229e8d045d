//go:build kzg_hip && !bignum_pure && !bignum_hol256 && !bignum_hbls
// +build kzg_hip,!bignum_pure,!bignum_hol256,!bignum_hbls

// The execution-layer side of eth/eth.go over many items in one device call: PointEvaluationPrecompileBatch (eth/eth.go:76-110),
// KZGToVersionedHashBatch (eth/eth.go:137-141) and VerifyKZGCommitmentsAgainstTransactionsBatch (eth/eth.go:234-282).  The lone calls stay
// where they are (INTEGRATION.md).
package eth

/*
#cgo LDFLAGS: -lkzg_hip
#include "kzg_hip.h"
*/
import "C"

import (
	"errors"
	"fmt"
	"unsafe"
)

// the result codes of include/kzg_hip.h (enum kzg_hip_eth_code)
const (
	hipEthInvalidProof  = 0
	hipEthValid         = 1
	hipEthBadField      = 2
	hipEthBadG1         = 3
	hipEthHashMismatch  = 4
	hipEthCountMismatch = 5
	hipEthTxTooShort    = 6
	hipEthTxOffset      = 7
	hipEthTxTrailing    = 8
)

// hands kzgSetupG2 to the eth handle once (as VerifyKZGProofBatch does)
func hipEnsureSetupG2() {
	hipSetupG2Mu.Lock()
	defer hipSetupG2Mu.Unlock()
	if hipSetupG2For != hipEth {
		if st := C.kzg_hip_eth_set_setup_g2(hipEth, unsafe.Pointer(&kzgSetupG2[0]), C.uint64_t(len(kzgSetupG2))); st != C.KZG_HIP_OK {
			panic("kzg_hip: eth_set_setup_g2 failed")
		}
		hipSetupG2For = hipEth
	}
}

// PrecompileReturnValueHip: precompileReturnValue (eth/globals.go:70-71) as the library states it for its handle
func PrecompileReturnValueHip() [64]byte {
	var out [64]byte
	if st := C.kzg_hip_eth_precompile_return_value(hipEth, unsafe.Pointer(&out[0])); st != C.KZG_HIP_OK {
		panic("kzg_hip: eth_precompile_return_value failed")
	}
	return out
}

// PointEvaluationPrecompileBatch: (outs[i], errs[i]) = PointEvaluationPrecompile(inputs[i]) with the reference's error texts.  An input whose
// length is not PrecompileInputLength gets "invalid input length" without going to the device.
func PointEvaluationPrecompileBatch(inputs [][]byte) ([][]byte, []error) {
	outs, errs := make([][]byte, len(inputs)), make([]error, len(inputs))
	var rows []int
	var flat []byte
	for i, in := range inputs {
		if len(in) != PrecompileInputLength {
			errs[i] = errors.New("invalid input length")
			continue
		}
		rows = append(rows, i)
		flat = append(flat, in...)
	}
	if len(rows) == 0 {
		return outs, errs
	}
	hipEnsureSetupG2()
	res := make([]uint8, len(rows))
	if st := C.kzg_hip_eth_point_evaluation_precompile_batch(hipEth, unsafe.Pointer(&flat[0]), C.uint64_t(len(rows)),
		(*C.uint8_t)(unsafe.Pointer(&res[0]))); st != C.KZG_HIP_OK {
		panic(fmt.Sprintf("kzg_hip: eth_point_evaluation_precompile_batch: status %d", int(st)))
	}
	for k, i := range rows {
		switch res[k] {
		case hipEthValid:
			result := precompileReturnValue // copy the value
			outs[i] = result[:]
		case hipEthInvalidProof:
			errs[i] = errInvalidKZGProof
		case hipEthHashMismatch:
			errs[i] = errors.New("mismatched versioned hash")
		default:
			// invalid inputs (the cold path): the reference's own parsing on the CPU names the input and the cause, with its error texts
			_, errs[i] = PointEvaluationPrecompile(inputs[i])
			if errs[i] == nil {
				panic("kzg_hip: eth_point_evaluation_precompile_batch rejected an input that PointEvaluationPrecompile accepts")
			}
		}
	}
	return outs, errs
}

// KZGToVersionedHashBatch: out[i] = KZGToVersionedHash(commitments[i])
func KZGToVersionedHashBatch(commitments []KZGCommitment) []VersionedHash {
	out := make([]VersionedHash, len(commitments))
	if len(commitments) == 0 {
		return out
	}
	if st := C.kzg_hip_eth_kzg_to_versioned_hash_batch(hipEth, unsafe.Pointer(&commitments[0]), C.uint64_t(len(commitments)),
		unsafe.Pointer(&out[0])); st != C.KZG_HIP_OK {
		panic(fmt.Sprintf("kzg_hip: eth_kzg_to_versioned_hash_batch: status %d", int(st)))
	}
	return out
}

// VerifyKZGCommitmentsAgainstTransactionsBatch: errs[j] = VerifyKZGCommitmentsAgainstTransactions(transactions[j], kzgCommitments[j]) for many
// blocks in one call.  A transaction of length 0, on which the reference panics, gets the "too short" error.
func VerifyKZGCommitmentsAgainstTransactionsBatch(transactions [][][]byte, kzgCommitments []KZGCommitmentSequence) []error {
	blocks := len(transactions)
	if len(kzgCommitments) != blocks {
		panic("VerifyKZGCommitmentsAgainstTransactionsBatch: slices of different lengths")
	}
	errs := make([]error, blocks)
	if blocks == 0 {
		return errs
	}
	txCounts, commCounts := make([]uint64, blocks), make([]uint64, blocks)
	offsets := []uint64{0}
	var txs []byte
	var comms []KZGCommitment
	for j := range transactions {
		txCounts[j] = uint64(len(transactions[j]))
		for _, tx := range transactions[j] {
			txs = append(txs, tx...)
			offsets = append(offsets, uint64(len(txs)))
		}
		commCounts[j] = uint64(kzgCommitments[j].Len())
		for i := 0; i < kzgCommitments[j].Len(); i++ {
			comms = append(comms, kzgCommitments[j].At(i))
		}
	}
	var tp, cp unsafe.Pointer
	if len(txs) > 0 {
		tp = unsafe.Pointer(&txs[0])
	}
	if len(comms) > 0 {
		cp = unsafe.Pointer(&comms[0])
	}
	res := make([]uint8, blocks)
	if st := C.kzg_hip_eth_verify_kzg_commitments_against_transactions_batch(hipEth, tp, (*C.uint64_t)(unsafe.Pointer(&offsets[0])),
		(*C.uint64_t)(unsafe.Pointer(&txCounts[0])), cp, (*C.uint64_t)(unsafe.Pointer(&commCounts[0])), C.uint64_t(blocks),
		(*C.uint8_t)(unsafe.Pointer(&res[0]))); st != C.KZG_HIP_OK {
		panic(fmt.Sprintf("kzg_hip: eth_verify_kzg_commitments_against_transactions_batch: status %d", int(st)))
	}
	for j, r := range res {
		switch r {
		case hipEthValid:
		case hipEthHashMismatch:
			errs[j] = errors.New("invalid version hashes vs kzg")
		case hipEthCountMismatch:
			found := 0
			for _, tx := range transactions[j] {
				if tx[0] == BlobTxType {
					v, _ := TxPeekBlobVersionedHashes(tx)
					found += len(v)
				}
			}
			errs[j] = fmt.Errorf("invalid number of blob versioned hashes: %v vs %v", kzgCommitments[j].Len(), found)
		case hipEthTxTooShort:
			errs[j] = errors.New("blob tx invalid: too short")
		case hipEthTxOffset:
			errs[j] = errors.New("offset to versioned hashes is out of bounds")
		case hipEthTxTrailing:
			errs[j] = errors.New("expected trailing data starting at versioned-hashes offset to be a multiple of 32 bytes")
		default:
			panic(fmt.Sprintf("kzg_hip: eth_verify_kzg_commitments_against_transactions_batch: code %d", int(r)))
		}
	}
	return errs
}
