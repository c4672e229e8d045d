//go:build kzg_hip && !bignum_pure && !bignum_hol256 && !bignum_hbls
// +build kzg_hip,!bignum_pure,!bignum_hol256,!bignum_hbls

// File for package bls (bls/pairing_hip.go): batch forms of bls.PairingsVerify, bls.FromCompressedG2, bls.ToCompressedG2 and
// bls.MulG2(.., &GenG2, ..) on the device.  The lone calls
// (PairingsVerify, FromCompressedG2) stay on Kilic: one check is one lane's work (INTEGRATION.md).  G2Point keeps Kilic's memory image,
// [3][2][6]uint64 Jacobian Montgomery, which is what the C ABI takes.
package bls

/*
#cgo LDFLAGS: -lkzg_hip
#include "kzg_hip.h"
*/
import "C"

import (
	"errors"
	"unsafe"
)

// PairingsVerifyBatch: out[i] = PairingsVerify(a1[i], a2[i], b1[i], b2[i]), all checks in one launch.
func PairingsVerifyBatch(a1 []G1Point, a2 []G2Point, b1 []G1Point, b2 []G2Point) []bool {
	n := len(a1)
	if len(a2) != n || len(b1) != n || len(b2) != n {
		panic("PairingsVerifyBatch: slices of different lengths")
	}
	out := make([]bool, n)
	if n == 0 {
		return out
	}
	ok := make([]uint8, n)
	st := C.kzg_hip_pairings_verify_batch(hipDomain(0), unsafe.Pointer(&a1[0]), unsafe.Pointer(&a2[0]), unsafe.Pointer(&b1[0]),
		unsafe.Pointer(&b2[0]), C.uint64_t(n), (*C.uint8_t)(unsafe.Pointer(&ok[0])))
	if st != C.KZG_HIP_OK {
		panic("kzg_hip: pairings_verify_batch failed")
	}
	for i := range ok {
		out[i] = ok[i] == 1
	}
	return out
}

// FromCompressedG2Batch: FromCompressedG2 over 96-byte encodings; an error if any encoding is invalid.
func FromCompressedG2Batch(in [][96]byte) ([]G2Point, error) {
	out := make([]G2Point, len(in))
	if len(in) == 0 {
		return out, nil
	}
	st := C.kzg_hip_g2_from_compressed(hipDomain(0), unsafe.Pointer(&in[0]), C.uint64_t(len(in)), unsafe.Pointer(&out[0]))
	if st == C.KZG_HIP_ERR_BAD_POINT {
		return nil, errors.New("invalid compressed G2 point")
	}
	if st != C.KZG_HIP_OK {
		panic("kzg_hip: g2_from_compressed failed")
	}
	return out, nil
}

// ToCompressedG2Batch: ToCompressedG2 over a slice (any Jacobian Z).  G2Point.MarshalText over a slice is hex.EncodeToString of each row.
func ToCompressedG2Batch(in []G2Point) [][96]byte {
	out := make([][96]byte, len(in))
	if len(in) == 0 {
		return out
	}
	st := C.kzg_hip_g2_to_compressed(hipDomain(0), unsafe.Pointer(&in[0]), C.uint64_t(len(in)), unsafe.Pointer(&out[0]))
	if st != C.KZG_HIP_OK {
		panic("kzg_hip: g2_to_compressed failed")
	}
	return out
}

// MulGenG2Batch: out[i] = MulG2(&GenG2, &scalars[i]) by a walk over the handle's table of GenG2, normalised (Z = 1).
func MulGenG2Batch(scalars []Fr) []G2Point {
	out := make([]G2Point, len(scalars))
	if len(scalars) == 0 {
		return out
	}
	st := C.kzg_hip_g2_mul_generator_vec(hipDomain(0), unsafe.Pointer(&scalars[0]), C.uint64_t(len(scalars)), unsafe.Pointer(&out[0]))
	if st != C.KZG_HIP_OK {
		panic("kzg_hip: g2_mul_generator_vec failed")
	}
	return out
}
