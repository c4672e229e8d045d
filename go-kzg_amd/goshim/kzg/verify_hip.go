//go:build kzg_hip && !bignum_pure && !bignum_hol256 && !bignum_hbls
// +build kzg_hip,!bignum_pure,!bignum_hol256,!bignum_hbls

// Batch forms of KZGSettings.CheckProofSingle / CheckProofMulti (kzg_single_proofs.go:57, kzg_multi_proofs.go:47) on the device.  The
// lone methods stay on Kilic (INTEGRATION.md).  ks.SecretG2 is handed to the device on the first batch check of a settings object.
package kzg

/*
#cgo LDFLAGS: -lkzg_hip
#include "kzg_hip.h"
*/
import "C"

import (
	"runtime"
	"unsafe"

	"github.com/protolambda/go-kzg/bls"
)

// hipSecretG2Set records, per settings object, the C handle that has received ks.SecretG2 (kzg_hip_kzg_set_secret_g2).  It lives under
// hipMu beside hipKZG and is cleared by CloseHip (hip_binding.go), so a handle made after an explicit close -- or for a new object at a
// reused address -- gets the array again.  The C side keeps each check's G2 state alive for the whole call, so even a redundant set
// racing with a check is safe; hipMu makes it happen once per handle.
var hipSecretG2Set = map[uintptr]*C.kzg_hip_kzg{}

func (ks *KZGSettings) hipSecretG2() *C.kzg_hip_kzg {
	h := ks.hip()
	key := uintptr(unsafe.Pointer(ks))
	hipMu.Lock()
	defer hipMu.Unlock()
	if hipSecretG2Set[key] != h {
		hipMust(C.kzg_hip_kzg_set_secret_g2(h, unsafe.Pointer(&ks.SecretG2[0]), C.uint64_t(len(ks.SecretG2))))
		hipSecretG2Set[key] = h
	}
	return h
}

func okMask(ok []uint8) []bool {
	out := make([]bool, len(ok))
	for i := range ok {
		out[i] = ok[i] == 1
	}
	return out
}

// CheckProofSingleBatch: out[i] = ks.CheckProofSingle(commitments[i], proofs[i], xs[i], ys[i]).
func (ks *KZGSettings) CheckProofSingleBatch(commitments, proofs []bls.G1Point, xs, ys []bls.Fr) []bool {
	defer runtime.KeepAlive(ks)
	n := len(commitments)
	if len(proofs) != n || len(xs) != n || len(ys) != n {
		panic("CheckProofSingleBatch: slices of different lengths")
	}
	if n == 0 {
		return nil
	}
	ok := make([]uint8, n)
	hipMust(C.kzg_hip_check_proof_single_batch(ks.hipSecretG2(), g1Ptr(commitments), g1Ptr(proofs), frPtr(xs), frPtr(ys), C.uint64_t(n),
		(*C.uint8_t)(unsafe.Pointer(&ok[0]))))
	return okMask(ok)
}

// CheckProofSingleBatchCombined: the mask of CheckProofSingleBatch with one pairing check per group of rows (a random linear combination per group;
// the rows of a failing group are re-checked one by one).  seed: nil draws the weights' seed from the operating system; 32 bytes make a run
// reproducible -- a seed the prover can know in advance voids the 2^-128 bound.  Presupposes points of G1, as CheckProofSingle does.
func (ks *KZGSettings) CheckProofSingleBatchCombined(commitments, proofs []bls.G1Point, xs, ys []bls.Fr, seed *[32]byte) []bool {
	defer runtime.KeepAlive(ks)
	n := len(commitments)
	if len(proofs) != n || len(xs) != n || len(ys) != n {
		panic("CheckProofSingleBatchCombined: slices of different lengths")
	}
	if n == 0 {
		return nil
	}
	var sp *C.uint8_t
	if seed != nil {
		sp = (*C.uint8_t)(unsafe.Pointer(&seed[0]))
	}
	ok := make([]uint8, n)
	hipMust(C.kzg_hip_check_proof_single_batch_combined(ks.hipSecretG2(), g1Ptr(commitments), g1Ptr(proofs), frPtr(xs), frPtr(ys), C.uint64_t(n), sp,
		(*C.uint8_t)(unsafe.Pointer(&ok[0]))))
	return okMask(ok)
}

// CheckProofMultiBatch: out[i] = ks.CheckProofMulti(commitments[i], proofs[i], xs[i], ys[i]); every ys[i] has the same length.
func (ks *KZGSettings) CheckProofMultiBatch(commitments, proofs []bls.G1Point, xs []bls.Fr, ys [][]bls.Fr) []bool {
	defer runtime.KeepAlive(ks)
	n := len(commitments)
	if len(proofs) != n || len(xs) != n || len(ys) != n {
		panic("CheckProofMultiBatch: slices of different lengths")
	}
	if n == 0 {
		return nil
	}
	m := len(ys[0])
	flat := make([]bls.Fr, 0, n*m)
	for _, row := range ys {
		if len(row) != m {
			panic("CheckProofMultiBatch: ys rows of different lengths")
		}
		flat = append(flat, row...)
	}
	ok := make([]uint8, n)
	hipMust(C.kzg_hip_check_proof_multi_batch(ks.hipSecretG2(), g1Ptr(commitments), g1Ptr(proofs), frPtr(xs), frPtr(flat), C.uint64_t(m),
		C.uint64_t(n), (*C.uint8_t)(unsafe.Pointer(&ok[0]))))
	return okMask(ok)
}

// CheckProofMultiBatchCombined: the mask of CheckProofMultiBatch with one pairing check per group of rows (the check a DAS sampler makes on
// the proofs of DAUsingFK20Multi; the rows of a failing group are re-checked one by one).  seed as CheckProofSingleBatchCombined: nil draws
// it from the operating system, a seed the prover can know in advance voids the 2^-128 bound.  Presupposes points of G1, as CheckProofMulti does.
func (ks *KZGSettings) CheckProofMultiBatchCombined(commitments, proofs []bls.G1Point, xs []bls.Fr, ys [][]bls.Fr, seed *[32]byte) []bool {
	defer runtime.KeepAlive(ks)
	n := len(commitments)
	if len(proofs) != n || len(xs) != n || len(ys) != n {
		panic("CheckProofMultiBatchCombined: slices of different lengths")
	}
	if n == 0 {
		return nil
	}
	m := len(ys[0])
	flat := make([]bls.Fr, 0, n*m)
	for _, row := range ys {
		if len(row) != m {
			panic("CheckProofMultiBatchCombined: ys rows of different lengths")
		}
		flat = append(flat, row...)
	}
	var sp *C.uint8_t
	if seed != nil {
		sp = (*C.uint8_t)(unsafe.Pointer(&seed[0]))
	}
	ok := make([]uint8, n)
	hipMust(C.kzg_hip_check_proof_multi_batch_combined(ks.hipSecretG2(), g1Ptr(commitments), g1Ptr(proofs), frPtr(xs), frPtr(flat), C.uint64_t(m),
		C.uint64_t(n), sp, (*C.uint8_t)(unsafe.Pointer(&ok[0]))))
	return okMask(ok)
}
