//go:build kzg_hip && !bignum_pure && !bignum_hol256 && !bignum_hbls
// +build kzg_hip,!bignum_pure,!bignum_hol256,!bignum_hbls

package kzg

/*
#include "kzg_hip.h"
*/
import "C"

import (
	"sync"
	"unsafe"

	"github.com/protolambda/go-kzg/bls"
)

var (
	hipCtxOnce sync.Once
	hipCtx     *C.kzg_hip_fft // scale-0 settings: a device context for calls that need no domain
)

func hipContext() *C.kzg_hip_fft {
	hipCtxOnce.Do(func() {
		hipMust(C.kzg_hip_fft_settings_new(C.int(HipDeviceID), 0, &hipCtx))
	})
	return hipCtx
}

// GenerateTestingSetup replaces setup.go:9-26 (**for testing purposes only**, as there).  Both halves run on the device: n fixed-base
// multiplications [secret^i]G1 and n more [secret^i]G2 -- 65 536 of each for the scale-16 FK20Multi configuration.  The G2 half walks a table of
// bls.GenG2 that the handle builds on its first use (32 mixed additions per point instead of bls.MulG2's double-and-add).
func GenerateTestingSetup(secret string, n uint64) ([]bls.G1Point, []bls.G2Point) {
	var s bls.Fr
	bls.SetFr(&s, secret)
	s1Out := make([]bls.G1Point, n, n)
	s2Out := make([]bls.G2Point, n, n)
	if n > 0 {
		hipMust(C.kzg_hip_generate_testing_setup_g1(hipContext(), frPtr([]bls.Fr{s}), C.uint64_t(n), g1Ptr(s1Out)))
		hipMust(C.kzg_hip_generate_testing_setup_g2(hipContext(), frPtr([]bls.Fr{s}), C.uint64_t(n), unsafe.Pointer(&s2Out[0])))
	}
	return s1Out, s2Out
}
