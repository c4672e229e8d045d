//go:build kzg_hip && !bignum_pure && !bignum_hol256 && !bignum_hbls
// +build kzg_hip,!bignum_pure,!bignum_hol256,!bignum_hbls

package kzg

/*
#include "kzg_hip.h"
*/
import "C"

import (
	"runtime"
	"errors"
	"unsafe"

	"github.com/protolambda/go-kzg/bls"
)

// ZeroPolyViaMultiplication replaces zero_poly.go:116-217: (evaluations, coefficients) of the vanishing polynomial.
func (fs *FFTSettings) ZeroPolyViaMultiplication(missingIndices []uint64, length uint64) ([]bls.Fr, []bls.Fr) {
	defer runtime.KeepAlive(fs) // the finalizer must not free the device handle under a running call
	zeroEval := make([]bls.Fr, length)
	zeroPoly := make([]bls.Fr, length)
	var idx *C.uint64_t
	if len(missingIndices) > 0 {
		idx = (*C.uint64_t)(unsafe.Pointer(&missingIndices[0]))
	}
	hipMust(C.kzg_hip_zero_poly_via_multiplication(fs.hip(), idx, C.uint64_t(len(missingIndices)), C.uint64_t(length),
		frPtr(zeroEval), frPtr(zeroPoly)))
	return zeroEval, zeroPoly
}

// RecoverPolyFromSamples replaces recover_from_samples.go:42-109.  The device path always uses ZeroPolyViaMultiplication as
// the zero-polynomial function (the only one the reference ships); samples[i] == nil marks a missing value.
func (fs *FFTSettings) RecoverPolyFromSamples(samples []*bls.Fr, zeroPolyFn ZeroPolyFn) ([]bls.Fr, error) {
	defer runtime.KeepAlive(fs) // the finalizer must not free the device handle under a running call
	n := len(samples)
	flat := make([]bls.Fr, n)
	present := make([]byte, n)
	for i, s := range samples {
		if s != nil {
			bls.CopyFr(&flat[i], s)
			present[i] = 1
		}
	}
	out := make([]bls.Fr, n)
	st := C.kzg_hip_recover_poly_from_samples(fs.hip(), frPtr(flat), (*C.uint8_t)(unsafe.Pointer(&present[0])), C.uint64_t(n), frPtr(out))
	if st == C.KZG_HIP_ERR_RECOVERY {
		return nil, errors.New("failed to reconstruct data correctly") // recover_from_samples.go:103-107
	}
	hipMust(st)
	return out, nil
}

// recoverBatch runs kzg_hip_recover_poly_from_samples_batch on flattened rows; presentRows is 1 (one mask for every row) or len(rows).
func (fs *FFTSettings) recoverBatch(flat []bls.Fr, present []byte, presentRows int, n int, rows int) ([][]bls.Fr, []error) {
	defer runtime.KeepAlive(fs) // the finalizer must not free the device handle under a running call
	out := make([]bls.Fr, rows*n)
	status := make([]byte, rows)
	res := make([][]bls.Fr, rows)
	errs := make([]error, rows)
	if rows == 0 || n == 0 {
		return res, errs
	}
	hipMust(C.kzg_hip_recover_poly_from_samples_batch(fs.hip(), frPtr(flat), (*C.uint8_t)(unsafe.Pointer(&present[0])), C.uint64_t(presentRows),
		C.uint64_t(n), C.uint64_t(rows), frPtr(out), (*C.uint8_t)(unsafe.Pointer(&status[0]))))
	for b := 0; b < rows; b++ {
		switch C.int(status[b]) {
		case C.KZG_HIP_OK:
			res[b] = out[b*n : (b+1)*n]
		case C.KZG_HIP_ERR_RECOVERY:
			errs[b] = errors.New("failed to reconstruct data correctly") // recover_from_samples.go:103-107
		default:
			errs[b] = errors.New("no sample present in this row")
		}
	}
	return res, errs
}

// RecoverPolyFromSamplesBatch is RecoverPolyFromSamples on every row (all of one length) in one device call; rows[b][i] == nil marks a
// missing value.  One error slot per row: a failed row returns nil, its neighbours are recovered.
func (fs *FFTSettings) RecoverPolyFromSamplesBatch(rows [][]*bls.Fr) ([][]bls.Fr, []error) {
	if len(rows) == 0 {
		return nil, nil
	}
	n := len(rows[0])
	flat := make([]bls.Fr, len(rows)*n)
	present := make([]byte, len(rows)*n)
	for b, row := range rows {
		if len(row) != n {
			panic("rows of different lengths")
		}
		for i, s := range row {
			if s != nil {
				bls.CopyFr(&flat[b*n+i], s)
				present[b*n+i] = 1
			}
		}
	}
	return fs.recoverBatch(flat, present, len(rows), n, len(rows))
}

// RecoverPolyFromSamplesBatchSharedMask is the same for rows that lost the same columns: present[i] == false marks column i as missing
// in every row, and one vanishing polynomial serves all of them.
func (fs *FFTSettings) RecoverPolyFromSamplesBatchSharedMask(rows [][]bls.Fr, present []bool) ([][]bls.Fr, []error) {
	if len(rows) == 0 {
		return nil, nil
	}
	n := len(present)
	flat := make([]bls.Fr, len(rows)*n)
	mask := make([]byte, n)
	for i, p := range present {
		if p {
			mask[i] = 1
		}
	}
	for b, row := range rows {
		if len(row) != n {
			panic("rows and mask of different lengths")
		}
		copy(flat[b*n:(b+1)*n], row)
	}
	return fs.recoverBatch(flat, mask, 1, n, len(rows))
}

// ZeroPolyViaMultiplicationBatch is ZeroPolyViaMultiplication for several erasure sets in one device call: per set the evaluations,
// the coefficients and nil, or an error for a set with `length` indices or more or an index beyond the domain.
func (fs *FFTSettings) ZeroPolyViaMultiplicationBatch(missingIndices [][]uint64, length uint64) ([][]bls.Fr, [][]bls.Fr, []error) {
	defer runtime.KeepAlive(fs) // the finalizer must not free the device handle under a running call
	sets := len(missingIndices)
	evals := make([][]bls.Fr, sets)
	polys := make([][]bls.Fr, sets)
	errs := make([]error, sets)
	if sets == 0 {
		return evals, polys, errs
	}
	offsets := make([]uint64, sets+1)
	flat := make([]uint64, 0, 1)
	for b, m := range missingIndices {
		flat = append(flat, m...)
		offsets[b+1] = uint64(len(flat))
	}
	flat = append(flat, 0) // never empty: a pointer for a call whose sets are all empty
	ev := make([]bls.Fr, uint64(sets)*length+1)
	zp := make([]bls.Fr, uint64(sets)*length+1)
	status := make([]byte, sets)
	hipMust(C.kzg_hip_zero_poly_via_multiplication_batch(fs.hip(), (*C.uint64_t)(unsafe.Pointer(&flat[0])), (*C.uint64_t)(unsafe.Pointer(&offsets[0])),
		C.uint64_t(sets), C.uint64_t(length), frPtr(ev), frPtr(zp), (*C.uint8_t)(unsafe.Pointer(&status[0]))))
	for b := 0; b < sets; b++ {
		if C.int(status[b]) != C.KZG_HIP_OK {
			errs[b] = errors.New("expected output smaller or equal to input length") // zero_poly.go:205-207
			continue
		}
		evals[b] = ev[uint64(b)*length : uint64(b+1)*length]
		polys[b] = zp[uint64(b)*length : uint64(b+1)*length]
	}
	return evals, polys, errs
}

// ComputeProofMulti replaces kzg_multi_proofs.go:13-44 (the reference's divisor, X^n, is kept as it is).
func (ks *KZGSettings) ComputeProofMulti(poly []bls.Fr, x uint64, n uint64) *bls.G1Point {
	defer runtime.KeepAlive(ks) // the finalizer must not free the device handle under a running call
	out := new(bls.G1Point)
	hipMust(C.kzg_hip_compute_proof_multi(ks.hip(), frPtr(poly), C.uint64_t(len(poly)), C.uint64_t(x), C.uint64_t(n), unsafePointerG1(out)))
	return out
}

// checkProofMultiProverHalf is the device half of CheckProofMulti (kzg_multi_proofs.go:47-75): [I(s)]_1 and x^n.  The two
// pairings stay on the CPU backend (bls.PairingsVerify).
func (ks *KZGSettings) checkProofMultiProverHalf(x *bls.Fr, ys []bls.Fr) (is1 bls.G1Point, xPow bls.Fr) {
	defer runtime.KeepAlive(ks) // the finalizer must not free the device handle under a running call
	hipMust(C.kzg_hip_check_proof_multi_interpolation(ks.hip(), frPtr(ys), C.uint64_t(len(ys)), unsafe.Pointer(x),
		unsafePointerG1(&is1), unsafe.Pointer(&xPow)))
	return
}

// FrFrom32Slice / FrTo32Slice: bls.FrFrom32 / bls.FrTo32 (bls/bignum_kilic.go:33-55) over a whole slice on the device.
func (fs *FFTSettings) FrFrom32Slice(in [][32]byte) (out []bls.Fr, ok bool) {
	defer runtime.KeepAlive(fs) // the finalizer must not free the device handle under a running call
	out = make([]bls.Fr, len(in))
	if len(in) == 0 {
		return out, true
	}
	var allOK C.int
	hipMust(C.kzg_hip_fr_from_le32(fs.hip(), unsafe.Pointer(&in[0]), C.uint64_t(len(in)), frPtr(out), &allOK))
	return out, allOK != 0
}

func (fs *FFTSettings) FrTo32Slice(in []bls.Fr) [][32]byte {
	defer runtime.KeepAlive(fs) // the finalizer must not free the device handle under a running call
	out := make([][32]byte, len(in))
	if len(in) > 0 {
		hipMust(C.kzg_hip_fr_to_le32(fs.hip(), frPtr(in), C.uint64_t(len(in)), unsafe.Pointer(&out[0])))
	}
	return out
}
