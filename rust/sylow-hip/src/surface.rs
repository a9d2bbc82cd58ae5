//! The rest of sylow's trait surface as batches (north_star: `GroupTrait`, `FieldExtensionTrait`): every entry point of
//! include/sylow_hip.h that lib.rs does not already wrap, as a thin typed function over `ffi::`.
//!
//! NOT COMPILED IN THE AUTHORING ENVIRONMENT (see lib.rs).  tests/test_rust_ffi.py checks every `ffi::` call below against the
//! generated declarations (name, arity) and fails when a header entry point is reached by no wrapper.
//!
//! Field elements cross as canonical little-endian words (`Fp::value().to_words()`, fields/fp.rs:232-234) and come back through
//! `Fp::new(U256::from_words(..))`; extension-field elements are `[u64; 8 / 24 / 48]` in the reference's nesting order (the types'
//! coefficients are private upstream, so the word arrays are the stable interchange form -- `fp2_words` etc. in lib.rs rebuild
//! sylow values from them where constructors exist).
use crate::device::{self, Device, DeviceBuf};
use crate::{ffi, first_failure, fp_from_words, messages, DeviceG1, DeviceG2, GtOut, HipError};
use crate::{download_g1, download_g2, gt_from_words, upload_g1, upload_g2};
use std::os::raw::c_void;
use std::ptr;
use sylow::{Fp, Fr, G1Affine, G1Projective, G2Affine, G2Projective};

type BinOp = unsafe extern "C" fn(*const u64, *const u64, *mut u64, usize, *mut c_void) -> i32;
type UnOp = unsafe extern "C" fn(*const u64, *mut u64, usize, *mut c_void) -> i32;

fn fp_words(a: &[Fp]) -> Vec<[u64; 4]> {
    a.iter().map(|x| x.value().to_words()).collect()
}
fn fr_words(a: &[Fr]) -> Vec<[u64; 4]> {
    a.iter().map(|x| x.value().to_words()).collect()
}

fn binop<const W: usize>(dev: &Device, f: BinOp, a: &[[u64; W]], b: &[[u64; W]]) -> Result<Vec<[u64; W]>, HipError> {
    assert_eq!(a.len(), b.len());
    let n = a.len();
    let (da, db, out) = (dev.upload_soa::<W>(a)?, dev.upload_soa::<W>(b)?, dev.alloc::<u64>(W * n)?);
    // SAFETY: three SoA arrays of W * n words each.
    device::check(unsafe { f(da.as_ptr(), db.as_ptr(), out.as_mut_ptr(), n, dev.stream) })?;
    Ok(dev.download_aos::<W>(&out, n)?)
}
fn unop<const W: usize>(dev: &Device, f: UnOp, a: &[[u64; W]]) -> Result<Vec<[u64; W]>, HipError> {
    let n = a.len();
    let (da, out) = (dev.upload_soa::<W>(a)?, dev.alloc::<u64>(W * n)?);
    // SAFETY: two SoA arrays of W * n words each.
    device::check(unsafe { f(da.as_ptr(), out.as_mut_ptr(), n, dev.stream) })?;
    Ok(dev.download_aos::<W>(&out, n)?)
}
fn to_fp(w: Vec<[u64; 4]>) -> Vec<Fp> {
    w.iter().map(|x| fp_from_words(x)).collect()
}

// ------------------------------------------------------------------ Fp / Fr: the operator bounds of FieldExtensionTrait (fp.rs:97-131)
/// Batched `Add / Sub / Mul for Fp` (fp.rs:304-347, 414-422), `square` (fp.rs:620-622), `Neg` (fp.rs:442-449), `inv` (fp.rs:418-433, inv(0) = 0).
pub fn fp_add_batch(dev: &Device, a: &[Fp], b: &[Fp]) -> Result<Vec<Fp>, HipError> {
    Ok(to_fp(binop::<4>(dev, ffi::sylow_hip_fp_add_batch, &fp_words(a), &fp_words(b))?))
}
pub fn fp_sub_batch(dev: &Device, a: &[Fp], b: &[Fp]) -> Result<Vec<Fp>, HipError> {
    Ok(to_fp(binop::<4>(dev, ffi::sylow_hip_fp_sub_batch, &fp_words(a), &fp_words(b))?))
}
pub fn fp_mul_batch(dev: &Device, a: &[Fp], b: &[Fp]) -> Result<Vec<Fp>, HipError> {
    Ok(to_fp(binop::<4>(dev, ffi::sylow_hip_fp_mul_batch, &fp_words(a), &fp_words(b))?))
}
pub fn fp_square_batch(dev: &Device, a: &[Fp]) -> Result<Vec<Fp>, HipError> {
    Ok(to_fp(unop::<4>(dev, ffi::sylow_hip_fp_sqr_batch, &fp_words(a))?))
}
pub fn fp_neg_batch(dev: &Device, a: &[Fp]) -> Result<Vec<Fp>, HipError> {
    Ok(to_fp(unop::<4>(dev, ffi::sylow_hip_fp_neg_batch, &fp_words(a))?))
}
pub fn fp_inv_batch(dev: &Device, a: &[Fp]) -> Result<Vec<Fp>, HipError> {
    Ok(to_fp(unop::<4>(dev, ffi::sylow_hip_fp_inv_batch, &fp_words(a))?))
}
/// `Fp::pow(U256)` (fp.rs:451-457); exponents as canonical words.
pub fn fp_pow_batch(dev: &Device, a: &[Fp], e: &[[u64; 4]]) -> Result<Vec<Fp>, HipError> {
    Ok(to_fp(binop::<4>(dev, ffi::sylow_hip_fp_pow_batch, &fp_words(a), e)?))
}
/// `Fp::sqrt` (fp.rs:611-616) as (candidate, is_some) and `Fp::is_square` (fp.rs:625-631).
pub fn fp_sqrt_batch(dev: &Device, a: &[Fp]) -> Result<Vec<Option<Fp>>, HipError> {
    let n = a.len();
    let (da, out, some) = (dev.upload_soa::<4>(&fp_words(a))?, dev.alloc::<u64>(4 * n)?, dev.alloc::<u8>(n)?);
    // SAFETY: 4 * n words in and out, n flags.
    device::check(unsafe { ffi::sylow_hip_fp_sqrt_batch(da.as_ptr(), out.as_mut_ptr(), some.as_mut_ptr(), n, dev.stream) })?;
    let (w, s) = (dev.download_aos::<4>(&out, n)?, dev.download(&some)?);
    Ok(w.iter().zip(s).map(|(x, ok)| if ok != 0 { Some(fp_from_words(x)) } else { None }).collect())
}
pub fn fp_is_square_batch(dev: &Device, a: &[Fp]) -> Result<Vec<bool>, HipError> {
    let n = a.len();
    let (da, flags) = (dev.upload_soa::<4>(&fp_words(a))?, dev.alloc::<u8>(n)?);
    // SAFETY: 4 * n words, n flags.
    device::check(unsafe { ffi::sylow_hip_fp_is_square_batch(da.as_ptr(), flags.as_mut_ptr(), n, dev.stream) })?;
    Ok(dev.download(&flags)?.iter().map(|&f| f != 0).collect())
}
/// `Fp::compute_naf` (fp.rs:653-662): the two 256-bit digit masks (plus, minus) of every scalar.
pub fn fp_compute_naf_batch(dev: &Device, k: &[Fp]) -> Result<Vec<([u64; 4], [u64; 4])>, HipError> {
    let n = k.len();
    let (dk, np, nm) = (dev.upload_soa::<4>(&fp_words(k))?, dev.alloc::<u64>(4 * n)?, dev.alloc::<u64>(4 * n)?);
    // SAFETY: three arrays of 4 * n words.
    device::check(unsafe { ffi::sylow_hip_fp_compute_naf_batch(dk.as_ptr(), np.as_mut_ptr(), nm.as_mut_ptr(), n, dev.stream) })?;
    Ok(dev.download_aos::<4>(&np, n)?.into_iter().zip(dev.download_aos::<4>(&nm, n)?).collect())
}
fn from_be_bytes(dev: &Device, fr: bool, blobs: &[[u8; 32]]) -> Result<Vec<Option<[u64; 4]>>, HipError> {
    let n = blobs.len();
    let flat: Vec<u8> = blobs.iter().flatten().copied().collect();
    let (d_in, out, st) = (dev.upload(&flat)?, dev.alloc::<u64>(4 * n)?, dev.alloc::<u8>(n)?);
    // SAFETY: 32 * n bytes in, 4 * n words and n status bytes out.
    device::check(unsafe {
        if fr {
            ffi::sylow_hip_fr_from_be_bytes_batch(d_in.as_ptr(), out.as_mut_ptr(), st.as_mut_ptr(), n, dev.stream)
        } else {
            ffi::sylow_hip_fp_from_be_bytes_batch(d_in.as_ptr(), out.as_mut_ptr(), st.as_mut_ptr(), n, dev.stream)
        }
    })?;
    let (w, s) = (dev.download_aos::<4>(&out, n)?, dev.download(&st)?);
    Ok(w.into_iter().zip(s).map(|(x, bad)| if bad == 0 { Some(x) } else { None }).collect())
}
/// `Fp::from_be_bytes` / `Fr::from_be_bytes` (fp.rs:686-719, 746-778): `None` where the value is not below the modulus.
pub fn fp_from_be_bytes_batch(dev: &Device, blobs: &[[u8; 32]]) -> Result<Vec<Option<Fp>>, HipError> {
    Ok(from_be_bytes(dev, false, blobs)?.into_iter().map(|o| o.map(|w| fp_from_words(&w))).collect())
}
pub fn fr_from_be_bytes_batch(dev: &Device, blobs: &[[u8; 32]]) -> Result<Vec<Option<[u64; 4]>>, HipError> {
    from_be_bytes(dev, true, blobs)
}
fn to_be_bytes(dev: &Device, fr: bool, words: &[[u64; 4]]) -> Result<Vec<[u8; 32]>, HipError> {
    let n = words.len();
    let (da, out) = (dev.upload_soa::<4>(words)?, dev.alloc::<u8>(32 * n)?);
    // SAFETY: 4 * n words in, 32 * n bytes out.
    device::check(unsafe {
        if fr {
            ffi::sylow_hip_fr_to_be_bytes_batch(da.as_ptr(), out.as_mut_ptr(), n, dev.stream)
        } else {
            ffi::sylow_hip_fp_to_be_bytes_batch(da.as_ptr(), out.as_mut_ptr(), n, dev.stream)
        }
    })?;
    Ok(dev.download(&out)?.chunks_exact(32).map(|c| c.try_into().unwrap()).collect())
}
/// `Fp::to_be_bytes` / `Fr::to_be_bytes` (fp.rs:727-737).
pub fn fp_to_be_bytes_batch(dev: &Device, a: &[Fp]) -> Result<Vec<[u8; 32]>, HipError> {
    to_be_bytes(dev, false, &fp_words(a))
}
pub fn fr_to_be_bytes_batch(dev: &Device, a: &[Fr]) -> Result<Vec<[u8; 32]>, HipError> {
    to_be_bytes(dev, true, &fr_words(a))
}
/// Fr arithmetic (fp.rs:556-565; Lagrange coefficients of examples/threshold_signing.rs:124-155), canonical words out.
pub fn fr_add_batch(dev: &Device, a: &[Fr], b: &[Fr]) -> Result<Vec<[u64; 4]>, HipError> {
    binop::<4>(dev, ffi::sylow_hip_fr_add_batch, &fr_words(a), &fr_words(b))
}
pub fn fr_sub_batch(dev: &Device, a: &[Fr], b: &[Fr]) -> Result<Vec<[u64; 4]>, HipError> {
    binop::<4>(dev, ffi::sylow_hip_fr_sub_batch, &fr_words(a), &fr_words(b))
}
pub fn fr_mul_batch(dev: &Device, a: &[Fr], b: &[Fr]) -> Result<Vec<[u64; 4]>, HipError> {
    binop::<4>(dev, ffi::sylow_hip_fr_mul_batch, &fr_words(a), &fr_words(b))
}
pub fn fr_square_batch(dev: &Device, a: &[Fr]) -> Result<Vec<[u64; 4]>, HipError> {
    unop::<4>(dev, ffi::sylow_hip_fr_sqr_batch, &fr_words(a))
}
pub fn fr_neg_batch(dev: &Device, a: &[Fr]) -> Result<Vec<[u64; 4]>, HipError> {
    unop::<4>(dev, ffi::sylow_hip_fr_neg_batch, &fr_words(a))
}
pub fn fr_inv_batch(dev: &Device, a: &[Fr]) -> Result<Vec<[u64; 4]>, HipError> {
    unop::<4>(dev, ffi::sylow_hip_fr_inv_batch, &fr_words(a))
}
/// The same words as `fr_inv_batch` (inv(0) = 0) by Montgomery's trick (`sylow_hip_fr_batch_inv`): the elements of a chunk of 2048 share ONE
/// inversion, about 5 products per element instead of a power per element.  The output is a buffer of its own, as the call requires.
pub fn fr_batch_inv(dev: &Device, a: &[Fr]) -> Result<Vec<[u64; 4]>, HipError> {
    unop::<4>(dev, ffi::sylow_hip_fr_batch_inv, &fr_words(a))
}

// ------------------------------------------------------------------ FieldExtension<D, N, F> (extensions.rs:41-238) and the tower
/// Component-wise `Add / Sub / Neg` and `scale(Fp)` of `FieldExtension` for degree 2, 6 or 12 (W = 4 * degree words per element).
pub fn fext_add_batch<const W: usize>(dev: &Device, a: &[[u64; W]], b: &[[u64; W]]) -> Result<Vec<[u64; W]>, HipError> {
    assert_eq!(a.len(), b.len());
    let n = a.len();
    let (da, db, out) = (dev.upload_soa::<W>(a)?, dev.upload_soa::<W>(b)?, dev.alloc::<u64>(W * n)?);
    // SAFETY: three SoA arrays of W * n words; degree = W / 4.
    device::check(unsafe { ffi::sylow_hip_fext_add_batch(da.as_ptr(), db.as_ptr(), out.as_mut_ptr(), (W / 4) as i32, n, dev.stream) })?;
    Ok(dev.download_aos::<W>(&out, n)?)
}
pub fn fext_sub_batch<const W: usize>(dev: &Device, a: &[[u64; W]], b: &[[u64; W]]) -> Result<Vec<[u64; W]>, HipError> {
    assert_eq!(a.len(), b.len());
    let n = a.len();
    let (da, db, out) = (dev.upload_soa::<W>(a)?, dev.upload_soa::<W>(b)?, dev.alloc::<u64>(W * n)?);
    // SAFETY: as fext_add_batch.
    device::check(unsafe { ffi::sylow_hip_fext_sub_batch(da.as_ptr(), db.as_ptr(), out.as_mut_ptr(), (W / 4) as i32, n, dev.stream) })?;
    Ok(dev.download_aos::<W>(&out, n)?)
}
pub fn fext_neg_batch<const W: usize>(dev: &Device, a: &[[u64; W]]) -> Result<Vec<[u64; W]>, HipError> {
    let n = a.len();
    let (da, out) = (dev.upload_soa::<W>(a)?, dev.alloc::<u64>(W * n)?);
    // SAFETY: two SoA arrays of W * n words.
    device::check(unsafe { ffi::sylow_hip_fext_neg_batch(da.as_ptr(), out.as_mut_ptr(), (W / 4) as i32, n, dev.stream) })?;
    Ok(dev.download_aos::<W>(&out, n)?)
}
pub fn fext_scale_batch<const W: usize>(dev: &Device, a: &[[u64; W]], k: &[Fp]) -> Result<Vec<[u64; W]>, HipError> {
    assert_eq!(a.len(), k.len());
    let n = a.len();
    let (da, dk, out) = (dev.upload_soa::<W>(a)?, dev.upload_soa::<4>(&fp_words(k))?, dev.alloc::<u64>(W * n)?);
    // SAFETY: W * n words in and out, 4 * n scalar words.
    device::check(unsafe { ffi::sylow_hip_fext_scale_batch(da.as_ptr(), dk.as_ptr(), out.as_mut_ptr(), (W / 4) as i32, n, dev.stream) })?;
    Ok(dev.download_aos::<W>(&out, n)?)
}
/// Fp2 (fp2.rs): `Mul`, `square`, `inv`, `residue_mul` (x (9 + u), :99-107), `frobenius(e)` (:119-133).
pub fn fp2_mul_batch(dev: &Device, a: &[[u64; 8]], b: &[[u64; 8]]) -> Result<Vec<[u64; 8]>, HipError> {
    binop::<8>(dev, ffi::sylow_hip_fp2_mul_batch, a, b)
}
pub fn fp2_square_batch(dev: &Device, a: &[[u64; 8]]) -> Result<Vec<[u64; 8]>, HipError> {
    unop::<8>(dev, ffi::sylow_hip_fp2_sqr_batch, a)
}
pub fn fp2_inv_batch(dev: &Device, a: &[[u64; 8]]) -> Result<Vec<[u64; 8]>, HipError> {
    unop::<8>(dev, ffi::sylow_hip_fp2_inv_batch, a)
}
pub fn fp2_residue_mul_batch(dev: &Device, a: &[[u64; 8]]) -> Result<Vec<[u64; 8]>, HipError> {
    unop::<8>(dev, ffi::sylow_hip_fp2_residue_mul_batch, a)
}
pub fn fp2_frobenius_batch(dev: &Device, a: &[[u64; 8]], exponent: usize) -> Result<Vec<[u64; 8]>, HipError> {
    let n = a.len();
    let (da, out) = (dev.upload_soa::<8>(a)?, dev.alloc::<u64>(8 * n)?);
    // SAFETY: two SoA arrays of 8 * n words.
    device::check(unsafe { ffi::sylow_hip_fp2_frobenius_batch(da.as_ptr(), exponent as u64, out.as_mut_ptr(), n, dev.stream) })?;
    Ok(dev.download_aos::<8>(&out, n)?)
}
/// Fp6 (fp6.rs): `Mul`, `square` (:213-236), `inv`, `residue_mul` (x v, :189-192), `frobenius(e)` (:205-211).
pub fn fp6_mul_batch(dev: &Device, a: &[[u64; 24]], b: &[[u64; 24]]) -> Result<Vec<[u64; 24]>, HipError> {
    binop::<24>(dev, ffi::sylow_hip_fp6_mul_batch, a, b)
}
pub fn fp6_square_batch(dev: &Device, a: &[[u64; 24]]) -> Result<Vec<[u64; 24]>, HipError> {
    unop::<24>(dev, ffi::sylow_hip_fp6_sqr_batch, a)
}
pub fn fp6_inv_batch(dev: &Device, a: &[[u64; 24]]) -> Result<Vec<[u64; 24]>, HipError> {
    unop::<24>(dev, ffi::sylow_hip_fp6_inv_batch, a)
}
pub fn fp6_residue_mul_batch(dev: &Device, a: &[[u64; 24]]) -> Result<Vec<[u64; 24]>, HipError> {
    unop::<24>(dev, ffi::sylow_hip_fp6_residue_mul_batch, a)
}
pub fn fp6_frobenius_batch(dev: &Device, a: &[[u64; 24]], exponent: usize) -> Result<Vec<[u64; 24]>, HipError> {
    let n = a.len();
    let (da, out) = (dev.upload_soa::<24>(a)?, dev.alloc::<u64>(24 * n)?);
    // SAFETY: two SoA arrays of 24 * n words.
    device::check(unsafe { ffi::sylow_hip_fp6_frobenius_batch(da.as_ptr(), exponent as u64, out.as_mut_ptr(), n, dev.stream) })?;
    Ok(dev.download_aos::<24>(&out, n)?)
}
/// Fp12 (fp12.rs): `Mul` (:229-238), `square` (:536-550), `inv` (:281-286), `frobenius(1..=3)` (:240-262), `sparse_mul` (:426-503),
/// and the Granger-Scott `cyclotomic_squared` of pairing.rs:309-350.
pub fn fp12_mul_batch(dev: &Device, a: &[[u64; 48]], b: &[[u64; 48]]) -> Result<Vec<[u64; 48]>, HipError> {
    binop::<48>(dev, ffi::sylow_hip_fp12_mul_batch, a, b)
}
pub fn fp12_square_batch(dev: &Device, a: &[[u64; 48]]) -> Result<Vec<[u64; 48]>, HipError> {
    unop::<48>(dev, ffi::sylow_hip_fp12_sqr_batch, a)
}
pub fn fp12_inv_batch(dev: &Device, a: &[[u64; 48]]) -> Result<Vec<[u64; 48]>, HipError> {
    unop::<48>(dev, ffi::sylow_hip_fp12_inv_batch, a)
}
pub fn fp12_cyclotomic_squared_batch(dev: &Device, a: &[[u64; 48]]) -> Result<Vec<[u64; 48]>, HipError> {
    unop::<48>(dev, ffi::sylow_hip_fp12_cyclotomic_sqr_batch, a)
}
pub fn fp12_frobenius_batch(dev: &Device, a: &[[u64; 48]], exponent: usize) -> Result<Vec<[u64; 48]>, HipError> {
    assert!((1..=3).contains(&exponent));
    let n = a.len();
    let (da, out) = (dev.upload_soa::<48>(a)?, dev.alloc::<u64>(48 * n)?);
    // SAFETY: two SoA arrays of 48 * n words.
    device::check(unsafe { ffi::sylow_hip_fp12_frobenius_batch(da.as_ptr(), exponent as i32, out.as_mut_ptr(), n, dev.stream) })?;
    Ok(dev.download_aos::<48>(&out, n)?)
}
/// `Fp12::sparse_mul(ell_0, ell_vw, ell_vv)`: `ell[i]` = the three Fp2 coefficients as 24 words.
pub fn fp12_sparse_mul_batch(dev: &Device, f: &[[u64; 48]], ell: &[[u64; 24]]) -> Result<Vec<[u64; 48]>, HipError> {
    assert_eq!(f.len(), ell.len());
    let n = f.len();
    let (df, dl, out) = (dev.upload_soa::<48>(f)?, dev.upload_soa::<24>(ell)?, dev.alloc::<u64>(48 * n)?);
    // SAFETY: 48 * n, 24 * n and 48 * n words.
    device::check(unsafe { ffi::sylow_hip_fp12_sparse_mul_batch(df.as_ptr(), dl.as_ptr(), out.as_mut_ptr(), n, dev.stream) })?;
    Ok(dev.download_aos::<48>(&out, n)?)
}
/// Raw selectors of the library's Fp / Fp12 test hooks (parity tests only; see include/sylow_hip.h for the op codes).
pub fn f29_hook_batch(dev: &Device, op: i32, a: &[[u64; 4]], b: &[[u64; 4]]) -> Result<Vec<[u64; 4]>, HipError> {
    assert_eq!(a.len(), b.len());
    let n = a.len();
    let (da, db, out) = (dev.upload_soa::<4>(a)?, dev.upload_soa::<4>(b)?, dev.alloc::<u64>(4 * n)?);
    // SAFETY: three SoA arrays of 4 * n words.
    device::check(unsafe { ffi::sylow_hip_f29_hook_batch(op, da.as_ptr(), db.as_ptr(), out.as_mut_ptr(), n, dev.stream) })?;
    Ok(dev.download_aos::<4>(&out, n)?)
}
/// Raw-limb test hook of the carry-free core: operands and output are `[i32; 9]` limb vectors, passed through unconverted (op codes in
/// include/sylow_hip.h; op 13 returns 18 limbs per element, the other ops 9).
pub fn f29_raw_hook_batch(dev: &Device, op: i32, ops: [Option<&[[i32; 9]]>; 4], k0: i32, k1: i32) -> Result<Vec<Vec<i32>>, HipError> {
    let n = ops[0].expect("operand a").len();
    let soa = |x: &[[i32; 9]]| -> Vec<i32> {
        assert_eq!(x.len(), n);
        (0..9).flat_map(|k| x.iter().map(move |e| e[k])).collect()
    };
    let mut bufs = Vec::new();
    for x in ops.iter() {
        bufs.push(match x {
            Some(x) => Some(dev.upload::<i32>(&soa(x))?),
            None => None,
        });
    }
    let w = if op == 13 { 18 } else { 9 };
    let out = dev.alloc::<i32>(w * n)?;
    let p = |i: usize| bufs[i].as_ref().map_or(ptr::null(), |d| d.as_ptr());
    // SAFETY: every operand present is 9 * n limbs, the output w * n (the width op 13 writes).
    device::check(unsafe { ffi::sylow_hip_f29_raw_hook_batch(op, p(0), p(1), p(2), p(3), k0, k1, out.as_mut_ptr(), n, dev.stream) })?;
    let flat = dev.download(&out)?;
    Ok((0..n).map(|i| (0..w).map(|k| flat[k * n + i]).collect()).collect())
}
pub fn fp12_hook_batch(dev: &Device, op: i32, a: &[[u64; 48]], b: Option<&[[u64; 48]]>) -> Result<Vec<[u64; 48]>, HipError> {
    let n = a.len();
    let da = dev.upload_soa::<48>(a)?;
    let db = match b {
        Some(b) => Some(dev.upload_soa::<48>(b)?),
        None => None,
    };
    let out = dev.alloc::<u64>(48 * n)?;
    // SAFETY: 48 * n words each; the second operand may be absent for unary selectors.
    device::check(unsafe {
        ffi::sylow_hip_fp12_hook_batch(op, da.as_ptr(), db.as_ref().map_or(ptr::null(), |d| d.as_ptr()), out.as_mut_ptr(), n, dev.stream)
    })?;
    Ok(dev.download_aos::<48>(&out, n)?)
}

// ------------------------------------------------------------------ GroupTrait (group.rs:60-164) and the group law
fn g1_pair_op(dev: &Device, which: u8, a: &[G1Affine], b: &[G1Affine]) -> Result<Vec<G1Projective>, HipError> {
    assert_eq!(a.len(), b.len());
    let n = a.len();
    let (da, db) = (upload_g1(dev, a)?, upload_g1(dev, b)?);
    let out = DeviceG1 { xy: dev.alloc::<u64>(8 * n)?, inf: dev.alloc::<u8>(n)?, n };
    // SAFETY: n affine points + flags on each side, n outputs.
    device::check(unsafe {
        if which == 0 {
            ffi::sylow_hip_g1_add_batch(da.xy.as_ptr(), da.inf.as_ptr(), db.xy.as_ptr(), db.inf.as_ptr(), out.xy.as_mut_ptr(), out.inf.as_mut_ptr(), n, dev.stream)
        } else {
            ffi::sylow_hip_g1_sub_batch(da.xy.as_ptr(), da.inf.as_ptr(), db.xy.as_ptr(), db.inf.as_ptr(), out.xy.as_mut_ptr(), out.inf.as_mut_ptr(), n, dev.stream)
        }
    })?;
    download_g1(dev, &out)
}
fn g2_pair_op(dev: &Device, which: u8, a: &[G2Affine], b: &[G2Affine]) -> Result<Vec<G2Projective>, HipError> {
    assert_eq!(a.len(), b.len());
    let n = a.len();
    let (da, db) = (upload_g2(dev, a)?, upload_g2(dev, b)?);
    let out = DeviceG2 { xy: dev.alloc::<u64>(16 * n)?, inf: dev.alloc::<u8>(n)?, n };
    // SAFETY: n affine points + flags on each side, n outputs.
    device::check(unsafe {
        if which == 0 {
            ffi::sylow_hip_g2_add_batch(da.xy.as_ptr(), da.inf.as_ptr(), db.xy.as_ptr(), db.inf.as_ptr(), out.xy.as_mut_ptr(), out.inf.as_mut_ptr(), n, dev.stream)
        } else {
            ffi::sylow_hip_g2_sub_batch(da.xy.as_ptr(), da.inf.as_ptr(), db.xy.as_ptr(), db.inf.as_ptr(), out.xy.as_mut_ptr(), out.inf.as_mut_ptr(), n, dev.stream)
        }
    })?;
    download_g2(dev, &out)
}
/// `Add` / `Sub` for `&G1Projective` and `&G2Projective` (group.rs:528-599, 614-624), `double` (group.rs:339-386).
pub fn g1_add_batch(dev: &Device, a: &[G1Affine], b: &[G1Affine]) -> Result<Vec<G1Projective>, HipError> {
    g1_pair_op(dev, 0, a, b)
}
pub fn g1_sub_batch(dev: &Device, a: &[G1Affine], b: &[G1Affine]) -> Result<Vec<G1Projective>, HipError> {
    g1_pair_op(dev, 1, a, b)
}
pub fn g2_add_batch(dev: &Device, a: &[G2Affine], b: &[G2Affine]) -> Result<Vec<G2Projective>, HipError> {
    g2_pair_op(dev, 0, a, b)
}
pub fn g2_sub_batch(dev: &Device, a: &[G2Affine], b: &[G2Affine]) -> Result<Vec<G2Projective>, HipError> {
    g2_pair_op(dev, 1, a, b)
}
pub fn g1_double_batch(dev: &Device, a: &[G1Affine]) -> Result<Vec<G1Projective>, HipError> {
    let n = a.len();
    let da = upload_g1(dev, a)?;
    let out = DeviceG1 { xy: dev.alloc::<u64>(8 * n)?, inf: dev.alloc::<u8>(n)?, n };
    // SAFETY: n points + flags in, n outputs.
    device::check(unsafe { ffi::sylow_hip_g1_double_batch(da.xy.as_ptr(), da.inf.as_ptr(), out.xy.as_mut_ptr(), out.inf.as_mut_ptr(), n, dev.stream) })?;
    download_g1(dev, &out)
}
pub fn g2_double_batch(dev: &Device, a: &[G2Affine]) -> Result<Vec<G2Projective>, HipError> {
    let n = a.len();
    let da = upload_g2(dev, a)?;
    let out = DeviceG2 { xy: dev.alloc::<u64>(16 * n)?, inf: dev.alloc::<u8>(n)?, n };
    // SAFETY: n points + flags in, n outputs.
    device::check(unsafe { ffi::sylow_hip_g2_double_batch(da.xy.as_ptr(), da.inf.as_ptr(), out.xy.as_mut_ptr(), out.inf.as_mut_ptr(), n, dev.stream) })?;
    download_g2(dev, &out)
}
/// `Mul<&Fp> for &G2Projective` for points that are NOT known to be in the r-torsion (generic window product, exact on the whole twist).
pub fn mul_g2_any_batch(dev: &Device, q: &DeviceG2, k: &[Fp]) -> Result<DeviceG2, HipError> {
    assert_eq!(q.n, k.len());
    let n = q.n;
    let dk = dev.upload_soa::<4>(&fp_words(k))?;
    let out = DeviceG2 { xy: dev.alloc::<u64>(16 * n)?, inf: dev.alloc::<u8>(n)?, n };
    // SAFETY: n points, 4 * n scalar words, n outputs.
    device::check(unsafe { ffi::sylow_hip_g2_scalar_mul_batch(q.xy.as_ptr(), q.inf.as_ptr(), dk.as_ptr(), out.xy.as_mut_ptr(), out.inf.as_mut_ptr(), n, dev.stream) })?;
    Ok(out)
}
/// `GroupTrait::rand` (g1.rs:293-305, g2.rs:227-240): generator * Fr::rand(rng), the scalars drawn on the host from the caller's generator.
pub fn g1_rand_batch<R: crypto_bigint::rand_core::CryptoRngCore>(dev: &Device, n: usize, rng: &mut R) -> Result<Vec<G1Projective>, HipError> {
    let k: Vec<[u64; 4]> = (0..n).map(|_| <Fr as sylow::FieldExtensionTrait<1, 1>>::rand(rng).value().to_words()).collect();
    let dk = dev.upload_soa::<4>(&k)?;
    let out = DeviceG1 { xy: dev.alloc::<u64>(8 * n)?, inf: dev.alloc::<u8>(n)?, n };
    // SAFETY: 4 * n scalar words, n outputs; the fixed-base table of the generator lives in the library.
    device::check(unsafe { ffi::sylow_hip_g1_generator_mul_batch(dk.as_ptr(), out.xy.as_mut_ptr(), out.inf.as_mut_ptr(), n, dev.stream) })?;
    download_g1(dev, &out)
}
pub fn g2_rand_batch<R: crypto_bigint::rand_core::CryptoRngCore>(dev: &Device, n: usize, rng: &mut R) -> Result<Vec<G2Projective>, HipError> {
    let k: Vec<Fp> = (0..n).map(|_| Fp::new(<Fr as sylow::FieldExtensionTrait<1, 1>>::rand(rng).value())).collect();
    crate::public_keys(dev, &k)
}
/// `GroupTrait::hash_to_curve` for G1 (g1.rs:307-331) with XMD-Keccak256 and sylow's DST (`dst = None`) or the caller's.
pub fn hash_to_curve_batch(dev: &Device, msgs: &[&[u8]], dst: Option<&[u8]>) -> Result<Vec<G1Projective>, HipError> {
    let n = msgs.len();
    let (d_msgs, d_off) = messages(dev, msgs)?;
    let out = DeviceG1 { xy: dev.alloc::<u64>(8 * n)?, inf: dev.alloc::<u8>(n)?, n };
    let (dst_ptr, dst_len) = dst.map_or((ptr::null(), 0), |d| (d.as_ptr(), d.len()));
    // SAFETY: n + 1 offsets into d_msgs; dst is a HOST pointer (read during the call); n outputs.
    device::check(unsafe { ffi::sylow_hip_hash_to_g1_batch(d_msgs.as_ptr(), d_off.as_ptr(), dst_ptr, dst_len, out.xy.as_mut_ptr(), out.inf.as_mut_ptr(), n, dev.stream) })?;
    download_g1(dev, &out)
}
/// `GroupTrait::sign_message` for G1 (g1.rs:355-366) = hash_to_curve(msg) * private_key: the batch is `sign_batch`.
pub fn sign_message_batch(dev: &Device, msgs: &[&[u8]], private_keys: &[Fp]) -> Result<Vec<G1Projective>, HipError> {
    crate::sign_batch(dev, private_keys, msgs)
}
/// `Expander::hash_to_field(msg, 2, 48)` (hasher.rs:84-128): two Fp per message.
pub fn hash_to_field_batch(dev: &Device, msgs: &[&[u8]], dst: Option<&[u8]>) -> Result<Vec<[Fp; 2]>, HipError> {
    let n = msgs.len();
    let (d_msgs, d_off) = messages(dev, msgs)?;
    let out = dev.alloc::<u64>(8 * n)?;
    let (dst_ptr, dst_len) = dst.map_or((ptr::null(), 0), |d| (d.as_ptr(), d.len()));
    // SAFETY: as hash_to_curve_batch; out holds 8 * n words.
    device::check(unsafe { ffi::sylow_hip_hash_to_field_batch(d_msgs.as_ptr(), d_off.as_ptr(), dst_ptr, dst_len, out.as_mut_ptr(), n, dev.stream) })?;
    Ok(dev.download_aos::<8>(&out, n)?.iter().map(|w| [fp_from_words(&w[0..4]), fp_from_words(&w[4..8])]).collect())
}
/// The expanders the library hashes with (`SYLOW_HIP_EXPANDER_*`): sylow's `XMDExpander<Keccak256>`, `XMDExpander<Sha256>` and
/// `XOFExpander<Shake128>` (lib.rs:71-84, hasher.rs:137-330), each with the caller's tag (`None` = sylow's DST) and security level k.
#[derive(Clone, Copy, PartialEq, Eq, Debug)]
pub enum Expander {
    XmdKeccak256 = 0,
    XmdSha256 = 1,
    XofShake128 = 2,
}
/// An `Expander` bound to its tag and security level: what `XMDExpander::new(dst, k)` / `XOFExpander::new(dst, k)` hold.
#[derive(Clone, Copy)]
pub struct Suite<'a> {
    pub expander: Expander,
    pub dst: Option<&'a [u8]>,
    pub security_bits: i32,
}
impl<'a> Suite<'a> {
    pub fn new(expander: Expander, dst: Option<&'a [u8]>) -> Self {
        Suite { expander, dst, security_bits: 128 }
    }
    fn dst_arg(&self) -> (*const u8, usize) {
        self.dst.map_or((ptr::null(), 0), |d| (d.as_ptr(), d.len()))
    }
}
/// `Expander::expand_message(msg, len_in_bytes)` (hasher.rs:201-250, 315-329): `len_in_bytes` bytes per message.  The conditions of
/// `HashError::ExpandMessage` fail the whole call.
pub fn expand_message_batch(dev: &Device, suite: &Suite, msgs: &[&[u8]], len_in_bytes: usize) -> Result<Vec<Vec<u8>>, HipError> {
    let n = msgs.len();
    let (d_msgs, d_off) = messages(dev, msgs)?;
    let out = dev.alloc::<u8>(len_in_bytes * n)?;
    let (dst_ptr, dst_len) = suite.dst_arg();
    // SAFETY: n + 1 offsets into d_msgs; dst is a HOST pointer (read during the call); out holds len_in_bytes * n bytes.
    device::check(unsafe {
        ffi::sylow_hip_expand_message_batch(suite.expander as i32, d_msgs.as_ptr(), d_off.as_ptr(), dst_ptr, dst_len, suite.security_bits, len_in_bytes,
                                            out.as_mut_ptr(), n, dev.stream)
    })?;
    let bytes = dev.download(&out)?;
    Ok(if len_in_bytes == 0 { vec![Vec::new(); n] } else { bytes.chunks(len_in_bytes).map(|c| c.to_vec()).collect() })
}
/// `Expander::hash_to_field(msg, 2, 48)` (hasher.rs:84-128) under the suite: two Fp per message.
pub fn hash_to_field_expander_batch(dev: &Device, suite: &Suite, msgs: &[&[u8]]) -> Result<Vec<[Fp; 2]>, HipError> {
    let n = msgs.len();
    let (d_msgs, d_off) = messages(dev, msgs)?;
    let out = dev.alloc::<u64>(8 * n)?;
    let (dst_ptr, dst_len) = suite.dst_arg();
    // SAFETY: as expand_message_batch; out holds 8 * n words.
    device::check(unsafe {
        ffi::sylow_hip_hash_to_field_expander_batch(suite.expander as i32, d_msgs.as_ptr(), d_off.as_ptr(), dst_ptr, dst_len, suite.security_bits,
                                                    out.as_mut_ptr(), n, dev.stream)
    })?;
    Ok(dev.download_aos::<8>(&out, n)?.iter().map(|w| [fp_from_words(&w[0..4]), fp_from_words(&w[4..8])]).collect())
}
/// `G1Projective::hash_to_curve(&expander, msg)` (g1.rs:307-331) under the suite.
pub fn hash_to_curve_expander_batch(dev: &Device, suite: &Suite, msgs: &[&[u8]]) -> Result<Vec<G1Projective>, HipError> {
    let n = msgs.len();
    let (d_msgs, d_off) = messages(dev, msgs)?;
    let out = DeviceG1 { xy: dev.alloc::<u64>(8 * n)?, inf: dev.alloc::<u8>(n)?, n };
    let (dst_ptr, dst_len) = suite.dst_arg();
    // SAFETY: as expand_message_batch; n outputs.
    device::check(unsafe {
        ffi::sylow_hip_hash_to_g1_expander_batch(suite.expander as i32, d_msgs.as_ptr(), d_off.as_ptr(), dst_ptr, dst_len, suite.security_bits,
                                                 out.xy.as_mut_ptr(), out.inf.as_mut_ptr(), n, dev.stream)
    })?;
    download_g1(dev, &out)
}
/// `GroupTrait::sign_message(&expander, msg, private_key)` (g1.rs:355-366) under the suite.
pub fn sign_message_expander_batch(dev: &Device, suite: &Suite, msgs: &[&[u8]], private_keys: &[Fp]) -> Result<Vec<G1Projective>, HipError> {
    assert_eq!(private_keys.len(), msgs.len());
    let n = msgs.len();
    let words: Vec<[u64; 4]> = private_keys.iter().map(|k| k.value().to_words()).collect();
    let d_sk = dev.upload_soa::<4>(&words)?;
    let (d_msgs, d_off) = messages(dev, msgs)?;
    let sig = DeviceG1 { xy: dev.alloc::<u64>(8 * n)?, inf: dev.alloc::<u8>(n)?, n };
    let (dst_ptr, dst_len) = suite.dst_arg();
    // SAFETY: sk 4 * n words, offsets n + 1 entries into d_msgs, outputs n elements; dst is a HOST pointer.
    device::check(unsafe {
        ffi::sylow_hip_bls_sign_expander_batch(suite.expander as i32, dst_ptr, dst_len, suite.security_bits, d_sk.as_ptr(), d_msgs.as_ptr(), d_off.as_ptr(),
                                               sig.xy.as_mut_ptr(), sig.inf.as_mut_ptr(), n, dev.stream)
    })?;
    download_g1(dev, &sig)
}
/// `sylow::verify` (lib.rs:223-236) with H from the suite: ok[i] = [ e(sig[i], G2gen) == e(H(msgs[i]), pk[i]) ].
pub fn verify_expander_batch(dev: &Device, suite: &Suite, pk: &[G2Affine], msgs: &[&[u8]], sig: &[G1Affine]) -> Result<Vec<bool>, HipError> {
    assert!(pk.len() == msgs.len() && sig.len() == msgs.len());
    let n = msgs.len();
    let (dpk, dsig) = (upload_g2(dev, pk)?, upload_g1(dev, sig)?);
    let (d_msgs, d_off) = messages(dev, msgs)?;
    let ok = dev.alloc::<u8>(n)?;
    let (dst_ptr, dst_len) = suite.dst_arg();
    // SAFETY: n keys, n signatures, n + 1 offsets, n flags; dst is a HOST pointer.
    device::check(unsafe {
        ffi::sylow_hip_bls_verify_expander_batch(suite.expander as i32, dst_ptr, dst_len, suite.security_bits, dpk.xy.as_ptr(), dpk.inf.as_ptr(),
                                                 d_msgs.as_ptr(), d_off.as_ptr(), dsig.xy.as_ptr(), dsig.inf.as_ptr(), ok.as_mut_ptr(), n, dev.stream)
    })?;
    Ok(dev.download(&ok)?.iter().map(|&f| f != 0).collect())
}
/// The same check on points the caller hashed (another hash-to-curve, or one hash against many signatures):
/// ok[i] = [ e(sig[i], G2gen) == e(h[i], pk[i]) ].
pub fn verify_hashed_batch(dev: &Device, pk: &[G2Affine], h: &[G1Affine], sig: &[G1Affine]) -> Result<Vec<bool>, HipError> {
    assert!(pk.len() == h.len() && sig.len() == h.len());
    let n = h.len();
    let (dpk, dh, dsig) = (upload_g2(dev, pk)?, upload_g1(dev, h)?, upload_g1(dev, sig)?);
    let ok = dev.alloc::<u8>(n)?;
    // SAFETY: n keys, n hashes, n signatures, n flags.
    device::check(unsafe {
        ffi::sylow_hip_bls_verify_hashed_batch(dpk.xy.as_ptr(), dpk.inf.as_ptr(), dh.xy.as_ptr(), dh.inf.as_ptr(), dsig.xy.as_ptr(), dsig.inf.as_ptr(),
                                               ok.as_mut_ptr(), n, dev.stream)
    })?;
    Ok(dev.download(&ok)?.iter().map(|&f| f != 0).collect())
}
/// `SvdW::unchecked_map_to_point` (svdw.rs:180-262): u -> (x, y) on E(Fp); `None` where the reference returns an error.
pub fn svdw_map_batch(dev: &Device, u: &[Fp]) -> Result<Vec<Option<[Fp; 2]>>, HipError> {
    let n = u.len();
    let (du, out, st) = (dev.upload_soa::<4>(&fp_words(u))?, dev.alloc::<u64>(8 * n)?, dev.alloc::<u8>(n)?);
    // SAFETY: 4 * n words in, 8 * n words and n status bytes out.
    device::check(unsafe { ffi::sylow_hip_svdw_map_batch(du.as_ptr(), out.as_mut_ptr(), st.as_mut_ptr(), n, dev.stream) })?;
    let (w, s) = (dev.download_aos::<8>(&out, n)?, dev.download(&st)?);
    Ok(w.iter().zip(s).map(|(x, bad)| if bad == 0 { Some([fp_from_words(&x[0..4]), fp_from_words(&x[4..8])]) } else { None }).collect())
}
/// `G2Affine::endomorphism` (g2.rs:140-152).  Where the reference panics (the image is off the curve) the element fails with NotOnCurve.
pub fn endomorphism_batch(dev: &Device, q: &DeviceG2) -> Result<DeviceG2, HipError> {
    let n = q.n;
    let out = DeviceG2 { xy: dev.alloc::<u64>(16 * n)?, inf: dev.alloc::<u8>(n)?, n };
    let st = dev.alloc::<u8>(n)?;
    // SAFETY: n points + flags in, n outputs + n status bytes.
    device::check(unsafe { ffi::sylow_hip_g2_psi_batch(q.xy.as_ptr(), q.inf.as_ptr(), out.xy.as_mut_ptr(), out.inf.as_mut_ptr(), st.as_mut_ptr(), n, dev.stream) })?;
    first_failure(&dev.download(&st)?)?;
    Ok(out)
}
/// `G1Affine::new` (g1.rs:111-132) / the r-torsion test of `G2Projective::new` (g2.rs:460-525) on device-resident affine points: status bytes.
pub fn g1_on_curve_batch(dev: &Device, p: &DeviceG1) -> Result<Vec<u8>, HipError> {
    let st = dev.alloc::<u8>(p.n)?;
    // SAFETY: n points + flags, n status bytes.
    device::check(unsafe { ffi::sylow_hip_g1_on_curve_batch(p.xy.as_ptr(), p.inf.as_ptr(), st.as_mut_ptr(), p.n, dev.stream) })?;
    Ok(dev.download(&st)?)
}
pub fn g2_subgroup_check_batch(dev: &Device, q: &DeviceG2) -> Result<Vec<u8>, HipError> {
    let st = dev.alloc::<u8>(q.n)?;
    // SAFETY: n points + flags, n status bytes.
    device::check(unsafe { ffi::sylow_hip_g2_subgroup_check_batch(q.xy.as_ptr(), q.inf.as_ptr(), st.as_mut_ptr(), q.n, dev.stream) })?;
    Ok(dev.download(&st)?)
}
/// `G1Projective::new([x, y, z])` (g1.rs:383-402) / `G2Projective::new([x, y, z])` (g2.rs:460-525) on raw projective words: status bytes.
pub fn g1_projective_new_batch(dev: &Device, xyz: &[[u64; 12]]) -> Result<Vec<u8>, HipError> {
    let n = xyz.len();
    let (d, st) = (dev.upload_soa::<12>(xyz)?, dev.alloc::<u8>(n)?);
    // SAFETY: 12 * n words, n status bytes.
    device::check(unsafe { ffi::sylow_hip_g1_projective_new_batch(d.as_ptr(), st.as_mut_ptr(), n, dev.stream) })?;
    Ok(dev.download(&st)?)
}
pub fn g2_projective_new_batch(dev: &Device, xyz: &[[u64; 24]]) -> Result<Vec<u8>, HipError> {
    let n = xyz.len();
    let (d, st) = (dev.upload_soa::<24>(xyz)?, dev.alloc::<u8>(n)?);
    // SAFETY: 24 * n words, n status bytes.
    device::check(unsafe { ffi::sylow_hip_g2_projective_new_batch(d.as_ptr(), st.as_mut_ptr(), n, dev.stream) })?;
    Ok(dev.download(&st)?)
}
/// `ConstantTimeEq` / `PartialEq` for projective points (group.rs:426-447) on raw projective words.
pub fn g1_ct_eq_batch(dev: &Device, a: &[[u64; 12]], b: &[[u64; 12]]) -> Result<Vec<bool>, HipError> {
    assert_eq!(a.len(), b.len());
    let n = a.len();
    let (da, db, eq) = (dev.upload_soa::<12>(a)?, dev.upload_soa::<12>(b)?, dev.alloc::<u8>(n)?);
    // SAFETY: 12 * n words on each side, n result bytes.
    device::check(unsafe { ffi::sylow_hip_g1_ct_eq_batch(da.as_ptr(), db.as_ptr(), eq.as_mut_ptr(), n, dev.stream) })?;
    Ok(dev.download(&eq)?.iter().map(|&f| f != 0).collect())
}
pub fn g2_ct_eq_batch(dev: &Device, a: &[[u64; 24]], b: &[[u64; 24]]) -> Result<Vec<bool>, HipError> {
    assert_eq!(a.len(), b.len());
    let n = a.len();
    let (da, db, eq) = (dev.upload_soa::<24>(a)?, dev.upload_soa::<24>(b)?, dev.alloc::<u8>(n)?);
    // SAFETY: 24 * n words on each side, n result bytes.
    device::check(unsafe { ffi::sylow_hip_g2_ct_eq_batch(da.as_ptr(), db.as_ptr(), eq.as_mut_ptr(), n, dev.stream) })?;
    Ok(dev.download(&eq)?.iter().map(|&f| f != 0).collect())
}
/// `GroupAffine::from(&GroupProjective)` (group.rs:475-495) on raw projective words: affine words + identity flag.
pub fn g1_normalize_batch(dev: &Device, xyz: &[[u64; 12]]) -> Result<DeviceG1, HipError> {
    let n = xyz.len();
    let d = dev.upload_soa::<12>(xyz)?;
    let out = DeviceG1 { xy: dev.alloc::<u64>(8 * n)?, inf: dev.alloc::<u8>(n)?, n };
    // SAFETY: 12 * n words in, n outputs.
    device::check(unsafe { ffi::sylow_hip_g1_normalize_batch(d.as_ptr(), out.xy.as_mut_ptr(), out.inf.as_mut_ptr(), n, dev.stream) })?;
    Ok(out)
}
pub fn g2_normalize_batch(dev: &Device, xyz: &[[u64; 24]]) -> Result<DeviceG2, HipError> {
    let n = xyz.len();
    let d = dev.upload_soa::<24>(xyz)?;
    let out = DeviceG2 { xy: dev.alloc::<u64>(16 * n)?, inf: dev.alloc::<u8>(n)?, n };
    // SAFETY: 24 * n words in, n outputs.
    device::check(unsafe { ffi::sylow_hip_g2_normalize_batch(d.as_ptr(), out.xy.as_mut_ptr(), out.inf.as_mut_ptr(), n, dev.stream) })?;
    Ok(out)
}
/// `to_be_bytes` of device-resident points (g1.rs:151-180, g2.rs:319-359).
pub fn g1_to_be_bytes_batch(dev: &Device, p: &DeviceG1) -> Result<Vec<[u8; 64]>, HipError> {
    let out = dev.alloc::<u8>(64 * p.n)?;
    // SAFETY: n points + flags, 64 * n bytes out.
    device::check(unsafe { ffi::sylow_hip_g1_to_be_bytes_batch(p.xy.as_ptr(), p.inf.as_ptr(), out.as_mut_ptr(), p.n, dev.stream) })?;
    Ok(dev.download(&out)?.chunks_exact(64).map(|c| c.try_into().unwrap()).collect())
}
pub fn g2_to_be_bytes_batch(dev: &Device, q: &DeviceG2) -> Result<Vec<[u8; 128]>, HipError> {
    let out = dev.alloc::<u8>(128 * q.n)?;
    // SAFETY: n points + flags, 128 * n bytes out.
    device::check(unsafe { ffi::sylow_hip_g2_to_be_bytes_batch(q.xy.as_ptr(), q.inf.as_ptr(), out.as_mut_ptr(), q.n, dev.stream) })?;
    Ok(dev.download(&out)?.chunks_exact(128).map(|c| c.try_into().unwrap()).collect())
}
/// Weighted aggregation sum_i weights[j][i] * points[j][i] (examples/threshold_signing.rs:124-143), term-major input:
/// element (job j, term i) at index i * n_jobs + j.
pub fn lincomb(dev: &Device, points: &[G1Affine], weights: &[Fr], n_jobs: usize, n_terms: usize) -> Result<Vec<G1Projective>, HipError> {
    assert!(points.len() == n_jobs * n_terms && weights.len() == points.len());
    let dp = upload_g1(dev, points)?;
    let dk = dev.upload_soa::<4>(&fr_words(weights))?;
    let out = DeviceG1 { xy: dev.alloc::<u64>(8 * n_jobs)?, inf: dev.alloc::<u8>(n_jobs)?, n: n_jobs };
    // SAFETY: n_jobs * n_terms points and scalars, n_jobs outputs.
    device::check(unsafe {
        ffi::sylow_hip_g1_lincomb_batch(dp.xy.as_ptr(), dp.inf.as_ptr(), dk.as_ptr(), out.xy.as_mut_ptr(), out.inf.as_mut_ptr(), n_jobs, n_terms, dev.stream)
    })?;
    download_g1(dev, &out)
}
/// sum_i scalars[i] * points[i] as one point by the bucket method (`sylow_hip_g1_msm`); the same point as
/// `lincomb(dev, points, scalars, 1, points.len())`.
pub fn msm(dev: &Device, points: &[G1Affine], scalars: &[Fr]) -> Result<G1Projective, HipError> {
    assert!(scalars.len() == points.len());
    let n = points.len();
    let dp = upload_g1(dev, points)?;
    let dk = dev.upload_soa::<4>(&fr_words(scalars))?;
    let out = DeviceG1 { xy: dev.alloc::<u64>(8)?, inf: dev.alloc::<u8>(1)?, n: 1 };
    // SAFETY: n points and scalars (possibly empty), one output point.
    device::check(unsafe {
        ffi::sylow_hip_g1_msm(dp.xy.as_ptr(), dp.inf.as_ptr(), dk.as_ptr(), n, out.xy.as_mut_ptr(), out.inf.as_mut_ptr(), dev.stream)
    })?;
    Ok(download_g1(dev, &out)?.remove(0))
}
/// `msm` with the plan pinned (`sylow_hip_g1_msm_tuned`): window width 4..16 and the smallest n on the bucket route; < 0 = the
/// defaults.  The point does not depend on either.
pub fn msm_tuned(dev: &Device, points: &[G1Affine], scalars: &[Fr], window: i32, min_n: i64) -> Result<G1Projective, HipError> {
    assert!(scalars.len() == points.len());
    let n = points.len();
    let dp = upload_g1(dev, points)?;
    let dk = dev.upload_soa::<4>(&fr_words(scalars))?;
    let out = DeviceG1 { xy: dev.alloc::<u64>(8)?, inf: dev.alloc::<u8>(1)?, n: 1 };
    // SAFETY: n points and scalars (possibly empty), one output point.
    device::check(unsafe {
        ffi::sylow_hip_g1_msm_tuned(dp.xy.as_ptr(), dp.inf.as_ptr(), dk.as_ptr(), n, window, min_n, out.xy.as_mut_ptr(), out.inf.as_mut_ptr(), dev.stream)
    })?;
    Ok(download_g1(dev, &out)?.remove(0))
}
/// `Mul<Fr> for Gt` (gt.rs:188-215): gt[i] ^ k[i], the reference's own 256-step signed-digit algorithm.
pub fn gt_pow_batch(dev: &Device, gt: &[[u64; 48]], k: &[Fr]) -> Result<Vec<GtOut>, HipError> {
    assert_eq!(gt.len(), k.len());
    let n = gt.len();
    let (dg, dk, out) = (dev.upload_soa::<48>(gt)?, dev.upload_soa::<4>(&fr_words(k))?, dev.alloc::<u64>(48 * n)?);
    // SAFETY: 48 * n words, 4 * n scalar words, 48 * n words out.
    device::check(unsafe { ffi::sylow_hip_gt_pow_batch(dg.as_ptr(), dk.as_ptr(), out.as_mut_ptr(), n, dev.stream) })?;
    Ok(dev.download_aos::<48>(&out, n)?.iter().map(gt_from_words).collect())
}

// ------------------------------------------------------------------ pairing.rs: the loops as entry points of their own
/// `G2PreComputed::miller_loop` / `glued_miller_loop` from the POINTS (lines computed on the fly): raw Miller values, 48 words each.
pub fn miller_loop_batch(dev: &Device, p: &DeviceG1, q: &DeviceG2) -> Result<DeviceBuf<u64>, HipError> {
    assert_eq!(p.n, q.n);
    let f = dev.alloc::<u64>(48 * p.n)?;
    // SAFETY: n points on each side, 48 * n words out.
    device::check(unsafe { ffi::sylow_hip_miller_loop_batch(p.xy.as_ptr(), q.xy.as_ptr(), f.as_mut_ptr(), p.n, dev.stream) })?;
    Ok(f)
}
/// Job j multiplies pairs [offsets[j], offsets[j+1]) with shared squarings (pairing.rs:970-1022); raw values out.
pub fn glued_miller_loop_batch(dev: &Device, p: &DeviceG1, q: &DeviceG2, offsets: &[u64]) -> Result<DeviceBuf<u64>, HipError> {
    assert!(p.n == q.n && !offsets.is_empty() && *offsets.last().unwrap() as usize <= p.n);
    let n_jobs = offsets.len() - 1;
    let (d_off, f) = (dev.upload(offsets)?, dev.alloc::<u64>(48 * n_jobs.max(1))?);
    // SAFETY: n pairs, n_jobs + 1 offsets, 48 * n_jobs words out.
    device::check(unsafe { ffi::sylow_hip_glued_miller_loop_batch(p.xy.as_ptr(), q.xy.as_ptr(), d_off.as_ptr(), n_jobs, p.n, f.as_mut_ptr(), dev.stream) })?;
    Ok(f)
}
/// `glued_pairing` per job (pairing.rs:1029-1037; the ecPairing / Groth16 shape): Gt values and `== identity` flags.
pub fn glued_pairing_jobs(dev: &Device, p: &DeviceG1, q: &DeviceG2, offsets: &[u64], skip_identity: bool) -> Result<(Vec<GtOut>, Vec<bool>), HipError> {
    assert!(p.n == q.n && !offsets.is_empty() && *offsets.last().unwrap() as usize <= p.n);
    let n_jobs = offsets.len() - 1;
    let (d_off, gt, one) = (dev.upload(offsets)?, dev.alloc::<u64>(48 * n_jobs.max(1))?, dev.alloc::<u8>(n_jobs.max(1))?);
    // SAFETY: n pairs + flags, n_jobs + 1 offsets, 48 * n_jobs words and n_jobs flags out.
    device::check(unsafe {
        ffi::sylow_hip_multi_pairing_batch(p.xy.as_ptr(), p.inf.as_ptr(), q.xy.as_ptr(), q.inf.as_ptr(), d_off.as_ptr(), n_jobs, p.n, skip_identity as i32,
                                           gt.as_mut_ptr(), one.as_mut_ptr(), dev.stream)
    })?;
    let words = dev.download_aos::<48>(&gt, n_jobs)?;
    Ok((words.iter().map(gt_from_words).collect(), dev.download(&one)?[..n_jobs].iter().map(|&f| f != 0).collect()))
}
/// `glued_miller_loop(&[G2PreComputed], &[G1Affine])` against tables `g2_precompute_batch` wrote (`coeffs` = [87 * 24][n_tables]).
pub fn glued_miller_loop_precomputed(dev: &Device, coeffs: &DeviceBuf<u64>, n_tables: usize, table_idx: &[u64], p: &DeviceG1, offsets: &[u64]) -> Result<DeviceBuf<u64>, HipError> {
    assert!(table_idx.len() == p.n && table_idx.iter().all(|&t| (t as usize) < n_tables));
    assert!(!offsets.is_empty() && *offsets.last().unwrap() as usize <= p.n);
    let n_jobs = offsets.len() - 1;
    let (d_idx, d_off, f) = (dev.upload(table_idx)?, dev.upload(offsets)?, dev.alloc::<u64>(48 * n_jobs.max(1))?);
    // SAFETY: n_tables tables, n indices < n_tables, n points, n_jobs + 1 offsets, 48 * n_jobs words out.
    device::check(unsafe {
        ffi::sylow_hip_glued_miller_loop_precomputed_batch(coeffs.as_ptr(), n_tables, d_idx.as_ptr(), p.xy.as_ptr(), d_off.as_ptr(), n_jobs, p.n, f.as_mut_ptr(), dev.stream)
    })?;
    Ok(f)
}
/// The two halves of a product split over GPUs by a host with its own transport: this shard's Miller product up to a factor in Fp*
/// (an opaque intermediate: the factor disappears in the final exponentiation; the reference's raw value comes from `miller_loop_batch`),
/// and product + final exponentiation over gathered partials (`parts` = [48][k] SoA).
pub fn pairing_product_partial(dev: &Device, p: &DeviceG1, q: &DeviceG2, skip_identity: bool) -> Result<DeviceBuf<u64>, HipError> {
    assert_eq!(p.n, q.n);
    let f = dev.alloc::<u64>(48)?;
    // SAFETY: n pairs + flags, 48 words out.
    device::check(unsafe {
        ffi::sylow_hip_pairing_product_partial_batch(p.xy.as_ptr(), p.inf.as_ptr(), q.xy.as_ptr(), q.inf.as_ptr(), p.n, skip_identity as i32, f.as_mut_ptr(), dev.stream)
    })?;
    Ok(f)
}
pub fn fp12_product_final_exp(dev: &Device, parts: &DeviceBuf<u64>, k: usize) -> Result<(GtOut, bool), HipError> {
    assert_eq!(parts.len, 48 * k);
    let (gt, one) = (dev.alloc::<u64>(48)?, dev.alloc::<u8>(1)?);
    // SAFETY: 48 * k words in, 48 words and one flag out.
    device::check(unsafe { ffi::sylow_hip_fp12_product_final_exp(parts.as_ptr(), k, gt.as_mut_ptr(), one.as_mut_ptr(), dev.stream) })?;
    let words = dev.download_aos::<48>(&gt, 1)?;
    Ok((gt_from_words(&words[0]), dev.download(&one)?[0] != 0))
}
/// This shard's Miller product (up to a factor in Fp*) of the aggregate check (signatures summed in G1 first), for a host-side gather.
pub fn aggregate_partial(dev: &Device, pk: &DeviceG2, msgs: &[&[u8]], sig: &DeviceG1) -> Result<DeviceBuf<u64>, HipError> {
    assert!(sig.n == msgs.len() && (pk.n == msgs.len() || pk.n == 1));
    let (d_msgs, d_off) = messages(dev, msgs)?;
    let f = dev.alloc::<u64>(48)?;
    // SAFETY: pk.n keys, n signatures, n + 1 offsets, 48 words out.
    device::check(unsafe {
        ffi::sylow_hip_bls_aggregate_partial_batch(pk.xy.as_ptr(), pk.inf.as_ptr(), pk.n, d_msgs.as_ptr(), d_off.as_ptr(), sig.xy.as_ptr(), sig.inf.as_ptr(), sig.n,
                                                   f.as_mut_ptr(), dev.stream)
    })?;
    Ok(f)
}
/// The SOUND one-boolean batch verification (small-exponent test): prod_i [e(sig_i, G2gen) e(-H(msg_i), pk_i)]^(w_i) == identity, with
/// `weights` drawn by the caller AFTER the signatures are fixed (e.g. 128 random bits each).  True when every signature is valid; a batch
/// with an invalid one passes with probability at most 2^-(bits of the weights).  `pk` one key per message or ONE key; `comm` as `all_valid`.
pub fn batch_verify_weighted(dev: &Device, pk: &DeviceG2, msgs: &[&[u8]], sig: &DeviceG1, weights: &[Fp], comm: *mut c_void) -> Result<(GtOut, bool), HipError> {
    assert!(sig.n == msgs.len() && weights.len() == msgs.len() && (pk.n == msgs.len() || pk.n == 1));
    let (d_msgs, d_off) = messages(dev, msgs)?;
    let dw = dev.upload_soa::<4>(&fp_words(weights))?;
    let (gt, one) = (dev.alloc::<u64>(48)?, dev.alloc::<u8>(1)?);
    // SAFETY: pk.n keys, n signatures, n + 1 offsets, 4 * n weight words; gt 48 words; one 1 byte; comm null or a live communicator.
    device::check(unsafe {
        ffi::sylow_hip_bls_batch_verify_weighted(pk.xy.as_ptr(), pk.inf.as_ptr(), pk.n, d_msgs.as_ptr(), d_off.as_ptr(), sig.xy.as_ptr(), sig.inf.as_ptr(),
                                                 dw.as_ptr(), sig.n, comm, gt.as_mut_ptr(), one.as_mut_ptr(), dev.stream)
    })?;
    let words = dev.download_aos::<48>(&gt, 1)?;
    Ok((gt_from_words(&words[0]), dev.download(&one)?[0] != 0))
}
/// This shard's Miller product (up to a factor in Fp*) of the weighted test, for a host-side gather (`fp12_product_final_exp` finishes it).
pub fn weighted_partial(dev: &Device, pk: &DeviceG2, msgs: &[&[u8]], sig: &DeviceG1, weights: &[Fp]) -> Result<DeviceBuf<u64>, HipError> {
    assert!(sig.n == msgs.len() && weights.len() == msgs.len() && (pk.n == msgs.len() || pk.n == 1));
    let (d_msgs, d_off) = messages(dev, msgs)?;
    let dw = dev.upload_soa::<4>(&fp_words(weights))?;
    let f = dev.alloc::<u64>(48)?;
    // SAFETY: as batch_verify_weighted; 48 words out.
    device::check(unsafe {
        ffi::sylow_hip_bls_weighted_partial_batch(pk.xy.as_ptr(), pk.inf.as_ptr(), pk.n, d_msgs.as_ptr(), d_off.as_ptr(), sig.xy.as_ptr(), sig.inf.as_ptr(),
                                                  dw.as_ptr(), sig.n, f.as_mut_ptr(), dev.stream)
    })?;
    Ok(f)
}
/// A Groth16 verifying key on the device: alpha (one G1 point), beta / gamma / delta (one G2 point each) and ic = IC_0 .. IC_l.  The
/// entry points take these arrays without flag arrays: a key's points are never the identity.
pub struct Groth16Vk {
    pub alpha: DeviceG1,
    pub beta: DeviceG2,
    pub gamma: DeviceG2,
    pub delta: DeviceG2,
    pub ic: DeviceG1,
}
impl Groth16Vk {
    /// l, the number of public inputs: ic holds IC_0 .. IC_l, at least IC_0
    pub fn n_inputs(&self) -> usize {
        assert!(self.ic.n >= 1, "a Groth16 key holds at least IC_0");
        self.ic.n - 1
    }
}
/// vk_x_i = IC_0 + sum_j x_ij IC_j for n proofs (`sylow_hip_groth16_vk_x_batch`).  `inputs` is INPUT-MAJOR: input j of proof i at index
/// j * n + i; any 256-bit words, taken mod r.
pub fn groth16_vk_x(dev: &Device, ic: &DeviceG1, inputs: &[Fr], n: usize) -> Result<DeviceG1, HipError> {
    assert!(ic.n >= 1, "ic holds at least IC_0");
    let n_inputs = ic.n - 1;
    assert!(inputs.len() == n_inputs * n);
    let dx = dev.upload_soa::<4>(&fr_words(inputs))?;
    let out = DeviceG1 { xy: dev.alloc::<u64>(8 * n)?, inf: dev.alloc::<u8>(n)?, n };
    // SAFETY: n_inputs + 1 bases, n_inputs * n input words, n outputs.
    device::check(unsafe { ffi::sylow_hip_groth16_vk_x_batch(ic.xy.as_ptr(), n_inputs, dx.as_ptr(), n, out.xy.as_mut_ptr(), out.inf.as_mut_ptr(), dev.stream) })?;
    Ok(out)
}
/// ok[i] = [ e(-A_i, B_i) e(alpha, beta) e(vk_x_i, gamma) e(C_i, delta) == 1 ] for n proofs under one key (`sylow_hip_groth16_verify_batch`);
/// identities follow EIP-197.  Precondition: B, beta, gamma, delta in G2 proper.  `inputs` input-major as for `groth16_vk_x`.
pub fn groth16_verify(dev: &Device, vk: &Groth16Vk, a: &DeviceG1, b: &DeviceG2, c: &DeviceG1, inputs: &[Fr]) -> Result<Vec<bool>, HipError> {
    let n = a.n;
    assert!(vk.ic.n >= 1 && b.n == n && c.n == n && inputs.len() == vk.n_inputs() * n);
    let dx = dev.upload_soa::<4>(&fr_words(inputs))?;
    let ok = dev.alloc::<u8>(n)?;
    // SAFETY: one point per vk array and n_inputs + 1 bases; n proofs with flags; n_inputs * n input words; n flags out.
    device::check(unsafe {
        ffi::sylow_hip_groth16_verify_batch(vk.alpha.xy.as_ptr(), vk.beta.xy.as_ptr(), vk.gamma.xy.as_ptr(), vk.delta.xy.as_ptr(), vk.ic.xy.as_ptr(), vk.n_inputs(),
                                            a.xy.as_ptr(), a.inf.as_ptr(), b.xy.as_ptr(), b.inf.as_ptr(), c.xy.as_ptr(), c.inf.as_ptr(), dx.as_ptr(), n,
                                            ok.as_mut_ptr(), dev.stream)
    })?;
    Ok(dev.download(&ok)?.into_iter().map(|v| v != 0).collect())
}
/// The SOUND one-boolean form for n Groth16 proofs (`sylow_hip_groth16_batch_verify_weighted`): `weights` drawn by the caller AFTER the
/// proofs are fixed (any 256-bit words, taken mod r; 0 removes a proof).  True when every proof is valid; a batch with an invalid one
/// passes with probability at most 2^-(bits of the weights), given G2 inputs in the r-torsion.
pub fn groth16_batch_verify_weighted(dev: &Device, vk: &Groth16Vk, a: &DeviceG1, b: &DeviceG2, c: &DeviceG1, inputs: &[Fr], weights: &[Fr]) -> Result<(GtOut, bool), HipError> {
    let n = a.n;
    assert!(vk.ic.n >= 1 && b.n == n && c.n == n && weights.len() == n && inputs.len() == vk.n_inputs() * n);
    let dx = dev.upload_soa::<4>(&fr_words(inputs))?;
    let dw = dev.upload_soa::<4>(&fr_words(weights))?;
    let (gt, one) = (dev.alloc::<u64>(48)?, dev.alloc::<u8>(1)?);
    // SAFETY: as groth16_verify, 4 * n weight words; gt 48 words; one 1 byte.
    device::check(unsafe {
        ffi::sylow_hip_groth16_batch_verify_weighted(vk.alpha.xy.as_ptr(), vk.beta.xy.as_ptr(), vk.gamma.xy.as_ptr(), vk.delta.xy.as_ptr(), vk.ic.xy.as_ptr(),
                                                     vk.n_inputs(), a.xy.as_ptr(), a.inf.as_ptr(), b.xy.as_ptr(), b.inf.as_ptr(), c.xy.as_ptr(), c.inf.as_ptr(),
                                                     dx.as_ptr(), dw.as_ptr(), n, gt.as_mut_ptr(), one.as_mut_ptr(), dev.stream)
    })?;
    let words = dev.download_aos::<48>(&gt, 1)?;
    Ok((gt_from_words(&words[0]), dev.download(&one)?[0] != 0))
}
/// The verifier's half of a BN254 KZG SRS on the device: tau_g2 = tau G2gen (one point of G2 proper, never the identity, so the entry points
/// take it without a flag array) and its line table, built once by `KzgSrs::new` and reused by every `kzg_verify`.
pub struct KzgSrs {
    pub tau_g2: DeviceG2,
    table: DeviceBuf<i32>,
}
impl KzgSrs {
    pub fn new(dev: &Device, tau_g2: DeviceG2) -> Result<Self, HipError> {
        assert!(tau_g2.n == 1, "tau_g2 is a single point");
        // SAFETY: no arguments.
        let words = unsafe { ffi::sylow_hip_g2_line_table_words() } as usize;
        let table = dev.alloc::<i32>(words)?;
        // SAFETY: tau_g2 is a 1-element SoA array; table holds `words` int32.
        device::check(unsafe { ffi::sylow_hip_g2_line_table(tau_g2.xy.as_ptr(), 1, 0, table.as_mut_ptr(), dev.stream) })?;
        dev.sync()?;
        Ok(KzgSrs { tau_g2, table })
    }
}
/// n KZG openings (C_i, z_i, y_i, pi_i), each claiming f(z_i) = y_i for the polynomial committed in C_i.  z and y are any 256-bit words,
/// taken mod r; a flagged C is the zero polynomial's commitment, a flagged pi the proof for a constant polynomial.
pub struct KzgOpenings<'a> {
    pub c: &'a DeviceG1,
    pub z: &'a [Fr],
    pub y: &'a [Fr],
    pub pi: &'a DeviceG1,
}
impl KzgOpenings<'_> {
    fn upload(&self, dev: &Device) -> Result<(usize, DeviceBuf<u64>, DeviceBuf<u64>), HipError> {
        let n = self.c.n;
        assert!(self.pi.n == n && self.z.len() == n && self.y.len() == n);
        Ok((n, dev.upload_soa::<4>(&fr_words(self.z))?, dev.upload_soa::<4>(&fr_words(self.y))?))
    }
}
/// F_i = C_i - y_i G1gen + z_i pi_i for every opening (`sylow_hip_kzg_fold_batch`): one launch, the identity as (0, 1) + flag.
pub fn kzg_fold(dev: &Device, o: &KzgOpenings) -> Result<DeviceG1, HipError> {
    let (n, dz, dy) = o.upload(dev)?;
    let out = DeviceG1 { xy: dev.alloc::<u64>(8 * n)?, inf: dev.alloc::<u8>(n)?, n };
    // SAFETY: n points with flags, 4 * n scalar words each, n outputs.
    device::check(unsafe {
        ffi::sylow_hip_kzg_fold_batch(o.c.xy.as_ptr(), o.c.inf.as_ptr(), dz.as_ptr(), dy.as_ptr(), o.pi.xy.as_ptr(), o.pi.inf.as_ptr(), out.xy.as_mut_ptr(),
                                      out.inf.as_mut_ptr(), n, dev.stream)
    })?;
    Ok(out)
}
/// ok[i] = [ e(C_i - y_i G1gen + z_i pi_i, G2gen) e(-pi_i, tau_g2) == 1 ] against the SRS's cached line table
/// (`sylow_hip_kzg_verify_line_table_batch`); identities follow EIP-197.
pub fn kzg_verify(dev: &Device, srs: &KzgSrs, o: &KzgOpenings) -> Result<Vec<bool>, HipError> {
    let (n, dz, dy) = o.upload(dev)?;
    let ok = dev.alloc::<u8>(n)?;
    // SAFETY: table built by KzgSrs::new on this device; n points with flags, 4 * n scalar words each, n flags out.
    device::check(unsafe {
        ffi::sylow_hip_kzg_verify_line_table_batch(srs.table.as_ptr(), o.c.xy.as_ptr(), o.c.inf.as_ptr(), dz.as_ptr(), dy.as_ptr(), o.pi.xy.as_ptr(), o.pi.inf.as_ptr(),
                                                   ok.as_mut_ptr(), n, dev.stream)
    })?;
    Ok(dev.download(&ok)?.into_iter().map(|v| v != 0).collect())
}
/// The same with the line table of tau_g2 built inside the call (`sylow_hip_kzg_verify_batch`): for a key used once.
pub fn kzg_verify_once(dev: &Device, tau_g2: &DeviceG2, o: &KzgOpenings) -> Result<Vec<bool>, HipError> {
    assert!(tau_g2.n == 1);
    let (n, dz, dy) = o.upload(dev)?;
    let ok = dev.alloc::<u8>(n)?;
    // SAFETY: one G2 point; n points with flags, 4 * n scalar words each, n flags out.
    device::check(unsafe {
        ffi::sylow_hip_kzg_verify_batch(tau_g2.xy.as_ptr(), o.c.xy.as_ptr(), o.c.inf.as_ptr(), dz.as_ptr(), dy.as_ptr(), o.pi.xy.as_ptr(), o.pi.inf.as_ptr(),
                                        ok.as_mut_ptr(), n, dev.stream)
    })?;
    Ok(dev.download(&ok)?.into_iter().map(|v| v != 0).collect())
}
/// The SOUND one-boolean form for n KZG openings (`sylow_hip_kzg_batch_verify_weighted`): `weights` drawn by the caller AFTER the openings
/// are fixed (any 256-bit words, taken mod r; 0 removes an opening).  True when every opening is valid; a batch with an invalid one passes
/// with probability at most 2^-(bits of the weights), given tau_g2 in the r-torsion.
pub fn kzg_batch_verify_weighted(dev: &Device, tau_g2: &DeviceG2, o: &KzgOpenings, weights: &[Fr]) -> Result<(GtOut, bool), HipError> {
    assert!(tau_g2.n == 1);
    let (n, dz, dy) = o.upload(dev)?;
    assert!(weights.len() == n);
    let dw = dev.upload_soa::<4>(&fr_words(weights))?;
    let (gt, one) = (dev.alloc::<u64>(48)?, dev.alloc::<u8>(1)?);
    // SAFETY: as kzg_verify_once, 4 * n weight words; gt 48 words; one 1 byte.
    device::check(unsafe {
        ffi::sylow_hip_kzg_batch_verify_weighted(tau_g2.xy.as_ptr(), o.c.xy.as_ptr(), o.c.inf.as_ptr(), dz.as_ptr(), dy.as_ptr(), o.pi.xy.as_ptr(), o.pi.inf.as_ptr(),
                                                 dw.as_ptr(), n, gt.as_mut_ptr(), one.as_mut_ptr(), dev.stream)
    })?;
    let words = dev.download_aos::<48>(&gt, 1)?;
    Ok((gt_from_words(&words[0]), dev.download(&one)?[0] != 0))
}
/// m polynomials of `len` coefficients each on the device, lowest degree first, in the block layout of the prover's calls: word w of
/// coefficient k of polynomial j at (j * 4 + w) * len + k.  Coefficients are any 256-bit words, taken mod r.
pub struct KzgPolys {
    pub words: DeviceBuf<u64>,
    pub len: usize,
    pub m: usize,
}
impl KzgPolys {
    /// `polys[j][k]` = coefficient k of polynomial j; every polynomial padded by the caller to the same length >= 1
    pub fn upload(dev: &Device, polys: &[Vec<Fr>]) -> Result<Self, HipError> {
        let (m, len) = (polys.len(), polys.first().map_or(1, |f| f.len()));
        assert!(len >= 1 && polys.iter().all(|f| f.len() == len), "polynomials are padded to one length >= 1");
        let mut flat = vec![0u64; 4 * len * m];
        for (j, f) in polys.iter().enumerate() {
            for (k, c) in fr_words(f).iter().enumerate() {
                for w in 0..4 {
                    flat[(j * 4 + w) * len + k] = c[w];
                }
            }
        }
        Ok(KzgPolys { words: dev.upload(&flat)?, len, m })
    }
}
/// The G1 half of a KZG SRS as the prover's calls take it: `srs.n` affine points tau^k G1gen, k = 0 .. n - 1, and polynomials of exactly
/// that many coefficients (a host with a longer SRS uploads a prefix).
fn kzg_srs_fits(srs: &DeviceG1, p: &KzgPolys) {
    assert!(srs.n == p.len, "the SRS holds one point per coefficient");
}
/// q_j = (f_j - f_j(z_j)) / (X - z_j) and y_j = f_j(z_j) (`sylow_hip_kzg_quotient_batch`): the quotients in the layout of `p`, y as [4][m] words.
pub fn kzg_quotient(dev: &Device, p: &KzgPolys, z: &[Fr]) -> Result<(KzgPolys, Vec<[u64; 4]>), HipError> {
    assert!(z.len() == p.m);
    let dz = dev.upload_soa::<4>(&fr_words(z))?;
    let (q, y) = (dev.alloc::<u64>(4 * p.len * p.m)?, dev.alloc::<u64>(4 * p.m)?);
    // SAFETY: m polynomials of len coefficients in and out (distinct buffers), 4 * m words of z and of y.
    device::check(unsafe { ffi::sylow_hip_kzg_quotient_batch(p.words.as_ptr(), p.len, p.m, dz.as_ptr(), q.as_mut_ptr(), y.as_mut_ptr(), dev.stream) })?;
    let yw = dev.download_aos::<4>(&y, p.m)?;
    Ok((KzgPolys { words: q, len: p.len, m: p.m }, yw))
}
/// y_j = f_j(z_j) alone: the same entry point without a quotient buffer.
pub fn kzg_evaluate(dev: &Device, p: &KzgPolys, z: &[Fr]) -> Result<Vec<[u64; 4]>, HipError> {
    assert!(z.len() == p.m);
    let dz = dev.upload_soa::<4>(&fr_words(z))?;
    let y = dev.alloc::<u64>(4 * p.m)?;
    // SAFETY: as kzg_quotient; a NULL q_out is the documented evaluation-only form.
    device::check(unsafe { ffi::sylow_hip_kzg_quotient_batch(p.words.as_ptr(), p.len, p.m, dz.as_ptr(), std::ptr::null_mut(), y.as_mut_ptr(), dev.stream) })?;
    Ok(dev.download_aos::<4>(&y, p.m)?)
}
/// C_j = sum_k f_jk srs_k for every polynomial (`sylow_hip_kzg_commit_batch`): m points, the identity as (0, 1) + flag.
pub fn kzg_commit(dev: &Device, srs: &DeviceG1, p: &KzgPolys) -> Result<DeviceG1, HipError> {
    kzg_srs_fits(srs, p);
    let out = DeviceG1 { xy: dev.alloc::<u64>(8 * p.m)?, inf: dev.alloc::<u8>(p.m)?, n: p.m };
    // SAFETY: len SRS points (no flags), m polynomials of len coefficients, m points and flags out.
    device::check(unsafe { ffi::sylow_hip_kzg_commit_batch(srs.xy.as_ptr(), p.words.as_ptr(), p.len, p.m, out.xy.as_mut_ptr(), out.inf.as_mut_ptr(), dev.stream) })?;
    Ok(out)
}
/// The same with the plan pinned (`sylow_hip_kzg_commit_batch_tuned`): `window` 4..16 for the bucket route, `min_len` the smallest length
/// that takes it; negative = the defaults.  The points do not depend on either.
pub fn kzg_commit_tuned(dev: &Device, srs: &DeviceG1, p: &KzgPolys, window: i32, min_len: i64) -> Result<DeviceG1, HipError> {
    kzg_srs_fits(srs, p);
    let out = DeviceG1 { xy: dev.alloc::<u64>(8 * p.m)?, inf: dev.alloc::<u8>(p.m)?, n: p.m };
    // SAFETY: as kzg_commit.
    device::check(unsafe {
        ffi::sylow_hip_kzg_commit_batch_tuned(srs.xy.as_ptr(), p.words.as_ptr(), p.len, p.m, window, min_len, out.xy.as_mut_ptr(), out.inf.as_mut_ptr(), dev.stream)
    })?;
    Ok(out)
}
/// The opening of every f_j at z_j (`sylow_hip_kzg_open_batch`): (y as [4][m] words, pi); pi_j is the identity exactly when f_j is constant.
pub fn kzg_open(dev: &Device, srs: &DeviceG1, p: &KzgPolys, z: &[Fr]) -> Result<(Vec<[u64; 4]>, DeviceG1), HipError> {
    kzg_srs_fits(srs, p);
    assert!(z.len() == p.m);
    let dz = dev.upload_soa::<4>(&fr_words(z))?;
    let y = dev.alloc::<u64>(4 * p.m)?;
    let pi = DeviceG1 { xy: dev.alloc::<u64>(8 * p.m)?, inf: dev.alloc::<u8>(p.m)?, n: p.m };
    // SAFETY: len SRS points, m polynomials of len coefficients, 4 * m words of z and of y, m points and flags out.
    device::check(unsafe {
        ffi::sylow_hip_kzg_open_batch(srs.xy.as_ptr(), p.words.as_ptr(), p.len, p.m, dz.as_ptr(), y.as_mut_ptr(), pi.xy.as_mut_ptr(), pi.inf.as_mut_ptr(), dev.stream)
    })?;
    Ok((dev.download_aos::<4>(&y, p.m)?, pi))
}
/// The commitments of m polynomials given by their VALUES on the domain of `srs.n` = 2^log_n points, `evals` in the layout of `KzgPolys` with
/// evals_ji = f_j(w_n^i) (`sylow_hip_kzg_commit_evals_batch`): word for word `kzg_commit` of the interpolated coefficients.
pub fn kzg_commit_evals(dev: &Device, srs: &DeviceG1, evals: &KzgPolys) -> Result<DeviceG1, HipError> {
    kzg_srs_fits(srs, evals);
    let log_n = radix2_log(evals.len);
    let out = DeviceG1 { xy: dev.alloc::<u64>(8 * evals.m)?, inf: dev.alloc::<u8>(evals.m)?, n: evals.m };
    // SAFETY: 2^log_n SRS points (no flags), m arrays of 2^log_n values, m points and flags out.
    device::check(unsafe {
        ffi::sylow_hip_kzg_commit_evals_batch(srs.xy.as_ptr(), evals.words.as_ptr(), log_n, evals.m, out.xy.as_mut_ptr(), out.inf.as_mut_ptr(), dev.stream)
    })?;
    Ok(out)
}
/// y_j = f_j(z_j) and the values on the domain of q_j = (f_j - y_j) / (X - z_j), from the VALUES evals_ji = f_j(w_n^i) in the layout of
/// `KzgPolys` (`sylow_hip_kzg_quotient_evals_batch`); z_j inside the domain is the documented 0 / 0 case, q_k = f_j'(w^k).  The quotients'
/// values in the layout of `evals`, y as [4][m] words.
pub fn kzg_quotient_evals(dev: &Device, evals: &KzgPolys, z: &[Fr]) -> Result<(KzgPolys, Vec<[u64; 4]>), HipError> {
    assert!(z.len() == evals.m);
    let log_n = radix2_log(evals.len);
    let dz = dev.upload_soa::<4>(&fr_words(z))?;
    let (q, y) = (dev.alloc::<u64>(4 * evals.len * evals.m)?, dev.alloc::<u64>(4 * evals.m)?);
    // SAFETY: m arrays of 2^log_n values in and out (distinct buffers), 4 * m words of z and of y.
    device::check(unsafe { ffi::sylow_hip_kzg_quotient_evals_batch(evals.words.as_ptr(), log_n, evals.m, dz.as_ptr(), q.as_mut_ptr(), y.as_mut_ptr(), dev.stream) })?;
    let yw = dev.download_aos::<4>(&y, evals.m)?;
    Ok((KzgPolys { words: q, len: evals.len, m: evals.m }, yw))
}
/// y_j = f_j(z_j) alone, by the barycentric formula: the same entry point without a quotient buffer.
pub fn kzg_evaluate_evals(dev: &Device, evals: &KzgPolys, z: &[Fr]) -> Result<Vec<[u64; 4]>, HipError> {
    assert!(z.len() == evals.m);
    let log_n = radix2_log(evals.len);
    let dz = dev.upload_soa::<4>(&fr_words(z))?;
    let y = dev.alloc::<u64>(4 * evals.m)?;
    // SAFETY: as kzg_quotient_evals; a NULL q_out is the documented evaluation-only form.
    device::check(unsafe {
        ffi::sylow_hip_kzg_quotient_evals_batch(evals.words.as_ptr(), log_n, evals.m, dz.as_ptr(), std::ptr::null_mut(), y.as_mut_ptr(), dev.stream)
    })?;
    Ok(dev.download_aos::<4>(&y, evals.m)?)
}
/// The opening of every f_j at z_j from its values, under the LAGRANGE-basis SRS of the same domain, `srs_lagrange.n` = 2^log_n points
/// L_i(tau) G1gen (`sylow_hip_kzg_open_evals_batch`): (y as [4][m] words, pi); pi_j is the identity exactly when f_j is constant.  The
/// commitment that goes with it is `kzg_commit(dev, srs_lagrange, evals)`.
pub fn kzg_open_evals(dev: &Device, srs_lagrange: &DeviceG1, evals: &KzgPolys, z: &[Fr]) -> Result<(Vec<[u64; 4]>, DeviceG1), HipError> {
    kzg_srs_fits(srs_lagrange, evals);
    assert!(z.len() == evals.m);
    let log_n = radix2_log(evals.len);
    let dz = dev.upload_soa::<4>(&fr_words(z))?;
    let y = dev.alloc::<u64>(4 * evals.m)?;
    let pi = DeviceG1 { xy: dev.alloc::<u64>(8 * evals.m)?, inf: dev.alloc::<u8>(evals.m)?, n: evals.m };
    // SAFETY: 2^log_n SRS points (no flags), m arrays of 2^log_n values, 4 * m words of z and of y, m points and flags out.
    device::check(unsafe {
        ffi::sylow_hip_kzg_open_evals_batch(srs_lagrange.xy.as_ptr(), evals.words.as_ptr(), log_n, evals.m, dz.as_ptr(), y.as_mut_ptr(), pi.xy.as_mut_ptr(),
                                            pi.inf.as_mut_ptr(), dev.stream)
    })?;
    Ok((dev.download_aos::<4>(&y, evals.m)?, pi))
}
/// Groups of consecutive polynomials for the folded openings: `offsets` holds G + 1 values, non-decreasing, from 0 to m; group g holds the
/// polynomials offsets[g] .. offsets[g + 1] - 1 (an empty group is legal).  A HOST array: the library reads it before a call returns.
pub struct KzgGroups {
    pub offsets: Vec<u64>,
}
impl KzgGroups {
    pub fn from_sizes(sizes: &[usize]) -> Self {
        let mut offsets = vec![0u64];
        for s in sizes {
            offsets.push(offsets[offsets.len() - 1] + *s as u64);
        }
        KzgGroups { offsets }
    }
    pub fn groups(&self) -> usize {
        self.offsets.len() - 1
    }
    fn fits(&self, m: usize) {
        assert!(self.offsets[0] == 0 && self.offsets[self.groups()] == m as u64 && self.offsets.windows(2).all(|w| w[0] <= w[1]), "offsets run from 0 to m");
    }
}
/// out_g = sum_{j in group g} weights_j a_j over Fr for m arrays in the layout of `KzgPolys` (`sylow_hip_fr_lincomb_batch`): G arrays.
pub fn fr_lincomb(dev: &Device, a: &KzgPolys, weights: &[Fr], groups: &KzgGroups) -> Result<KzgPolys, HipError> {
    groups.fits(a.m);
    assert!(weights.len() == a.m);
    let g = groups.groups();
    let dw = dev.upload_soa::<4>(&fr_words(weights))?;
    let out = dev.alloc::<u64>(4 * a.len * g)?;
    // SAFETY: m arrays of len words x 4 in, 4 * m weight words, G + 1 host offsets, G arrays out in a buffer of their own.
    device::check(unsafe { ffi::sylow_hip_fr_lincomb_batch(a.words.as_ptr(), a.len, a.m, dw.as_ptr(), groups.offsets.as_ptr(), g, out.as_mut_ptr(), dev.stream) })?;
    Ok(KzgPolys { words: out, len: a.len, m: g })
}
/// gamma_g^i for polynomial i of group g, as [4][m] words on the host (`sylow_hip_fr_group_powers_batch`).
pub fn fr_group_powers(dev: &Device, gamma: &[Fr], groups: &KzgGroups, m: usize) -> Result<Vec<[u64; 4]>, HipError> {
    groups.fits(m);
    let g = groups.groups();
    assert!(gamma.len() == g);
    let dg = dev.upload_soa::<4>(&fr_words(gamma))?;
    let out = dev.alloc::<u64>(4 * m)?;
    // SAFETY: 4 * G words of gamma, G + 1 host offsets, 4 * m words out.
    device::check(unsafe { ffi::sylow_hip_fr_group_powers_batch(dg.as_ptr(), groups.offsets.as_ptr(), g, m, out.as_mut_ptr(), dev.stream) })?;
    Ok(dev.download_aos::<4>(&out, m)?)
}
/// Every group of polynomials opened at its point z_g under ONE proof folded with gamma_g (`sylow_hip_kzg_open_multi_batch`): (y as [4][m]
/// words, the G proofs).  gamma is drawn by the caller AFTER the commitments and the claimed values are fixed.
pub fn kzg_open_multi(dev: &Device, srs: &DeviceG1, p: &KzgPolys, groups: &KzgGroups, z: &[Fr], gamma: &[Fr]) -> Result<(Vec<[u64; 4]>, DeviceG1), HipError> {
    kzg_srs_fits(srs, p);
    groups.fits(p.m);
    let g = groups.groups();
    assert!(z.len() == g && gamma.len() == g);
    let (dz, dg) = (dev.upload_soa::<4>(&fr_words(z))?, dev.upload_soa::<4>(&fr_words(gamma))?);
    let y = dev.alloc::<u64>(4 * p.m)?;
    let pi = DeviceG1 { xy: dev.alloc::<u64>(8 * g)?, inf: dev.alloc::<u8>(g)?, n: g };
    // SAFETY: len SRS points, m polynomials of len coefficients, G + 1 host offsets, 4 * G words of z and gamma, 4 * m words of y, G points and flags out.
    device::check(unsafe {
        ffi::sylow_hip_kzg_open_multi_batch(srs.xy.as_ptr(), p.words.as_ptr(), p.len, p.m, groups.offsets.as_ptr(), g, dz.as_ptr(), dg.as_ptr(), y.as_mut_ptr(),
                                            pi.xy.as_mut_ptr(), pi.inf.as_mut_ptr(), dev.stream)
    })?;
    Ok((dev.download_aos::<4>(&y, p.m)?, pi))
}
/// The same from evaluation form under the Lagrange-basis SRS (`sylow_hip_kzg_open_multi_evals_batch`).
pub fn kzg_open_multi_evals(dev: &Device, srs_lagrange: &DeviceG1, evals: &KzgPolys, groups: &KzgGroups, z: &[Fr], gamma: &[Fr])
                            -> Result<(Vec<[u64; 4]>, DeviceG1), HipError> {
    kzg_srs_fits(srs_lagrange, evals);
    groups.fits(evals.m);
    let g = groups.groups();
    assert!(z.len() == g && gamma.len() == g);
    let log_n = radix2_log(evals.len);
    let (dz, dg) = (dev.upload_soa::<4>(&fr_words(z))?, dev.upload_soa::<4>(&fr_words(gamma))?);
    let y = dev.alloc::<u64>(4 * evals.m)?;
    let pi = DeviceG1 { xy: dev.alloc::<u64>(8 * g)?, inf: dev.alloc::<u8>(g)?, n: g };
    // SAFETY: as kzg_open_multi with 2^log_n values per polynomial.
    device::check(unsafe {
        ffi::sylow_hip_kzg_open_multi_evals_batch(srs_lagrange.xy.as_ptr(), evals.words.as_ptr(), log_n, evals.m, groups.offsets.as_ptr(), g, dz.as_ptr(),
                                                  dg.as_ptr(), y.as_mut_ptr(), pi.xy.as_mut_ptr(), pi.inf.as_mut_ptr(), dev.stream)
    })?;
    Ok((dev.download_aos::<4>(&y, evals.m)?, pi))
}
/// The verifier's folded rows (`sylow_hip_kzg_combine_openings_batch`): C_F,g = sum_j gamma_g^i C_j and y_F,g = sum_j gamma_g^i y_j as
/// [4][G] device words -- with z and the proofs, the rows `kzg_verify_once` and `kzg_batch_verify_weighted` take.
pub fn kzg_combine_openings(dev: &Device, c: &DeviceG1, y: &[Fr], groups: &KzgGroups, gamma: &[Fr]) -> Result<(DeviceG1, DeviceBuf<u64>), HipError> {
    let m = c.n;
    groups.fits(m);
    let g = groups.groups();
    assert!(y.len() == m && gamma.len() == g);
    let (dy, dg) = (dev.upload_soa::<4>(&fr_words(y))?, dev.upload_soa::<4>(&fr_words(gamma))?);
    let cf = DeviceG1 { xy: dev.alloc::<u64>(8 * g)?, inf: dev.alloc::<u8>(g)?, n: g };
    let yf = dev.alloc::<u64>(4 * g)?;
    // SAFETY: m points with flags, 4 * m words of y, G + 1 host offsets, 4 * G words of gamma, G points, flags and values out.
    device::check(unsafe {
        ffi::sylow_hip_kzg_combine_openings_batch(c.xy.as_ptr(), c.inf.as_ptr(), dy.as_ptr(), m, groups.offsets.as_ptr(), g, dg.as_ptr(), cf.xy.as_mut_ptr(),
                                                  cf.inf.as_mut_ptr(), yf.as_mut_ptr(), dev.stream)
    })?;
    Ok((cf, yf))
}
/// ok[g] for every folded row (`sylow_hip_kzg_verify_multi_batch`): the combination, then the per-opening check over the G rows.
pub fn kzg_verify_multi(dev: &Device, tau_g2: &DeviceG2, c: &DeviceG1, y: &[Fr], groups: &KzgGroups, z: &[Fr], gamma: &[Fr], pi: &DeviceG1)
                        -> Result<Vec<bool>, HipError> {
    let m = c.n;
    groups.fits(m);
    let g = groups.groups();
    assert!(tau_g2.n == 1 && y.len() == m && z.len() == g && gamma.len() == g && pi.n == g);
    let (dy, dz, dg) = (dev.upload_soa::<4>(&fr_words(y))?, dev.upload_soa::<4>(&fr_words(z))?, dev.upload_soa::<4>(&fr_words(gamma))?);
    let ok = dev.alloc::<u8>(g)?;
    // SAFETY: one G2 point; m points with flags, 4 * m words of y, G + 1 host offsets, 4 * G words of z and gamma, G proofs with flags, G flags out.
    device::check(unsafe {
        ffi::sylow_hip_kzg_verify_multi_batch(tau_g2.xy.as_ptr(), c.xy.as_ptr(), c.inf.as_ptr(), dy.as_ptr(), m, groups.offsets.as_ptr(), g, dz.as_ptr(), dg.as_ptr(),
                                              pi.xy.as_ptr(), pi.inf.as_ptr(), ok.as_mut_ptr(), dev.stream)
    })?;
    Ok(dev.download(&ok)?.into_iter().map(|v| v != 0).collect())
}
/// log2 of a radix-2 domain's size (at most 2^28 points: r - 1 = 2^28 * odd)
fn radix2_log(n: usize) -> i32 {
    assert!(n.is_power_of_two() && n <= 1 << 28, "a radix-2 domain of at most 2^28 points");
    n.trailing_zeros() as i32
}
/// The transform over Fr of m arrays of n = 2^log_n elements in the layout of `KzgPolys` (`sylow_hip_fr_ntt_batch`), natural order in and out:
/// forward out_i = sum_k a_k (g w_n^i)^k, inverse out_k = n^-1 g^-k sum_i a_i w_n^(-ik); `shift` is the coset shift g (None: 1).  Any
/// 256-bit words in, taken mod r; canonical words out, in a buffer of their own.
pub fn fr_ntt(dev: &Device, a: &KzgPolys, inverse: bool, shift: Option<&Fr>) -> Result<KzgPolys, HipError> {
    let log_n = radix2_log(a.len);
    let dsh = match shift {
        Some(g) => Some(dev.upload_soa::<4>(&fr_words(std::slice::from_ref(g)))?),
        None => None,
    };
    let psh = dsh.as_ref().map_or(std::ptr::null(), |d| d.as_ptr());
    let out = dev.alloc::<u64>(4 * (1 << log_n) * a.m)?;
    // SAFETY: m arrays of 2^log_n elements in and out (distinct buffers), 4 words of shift or NULL.
    device::check(unsafe { ffi::sylow_hip_fr_ntt_batch(a.words.as_ptr(), log_n, a.m, inverse as i32, psh, out.as_mut_ptr(), dev.stream) })?;
    Ok(KzgPolys { words: out, len: a.len, m: a.m })
}
/// The same with the stages of a pass pinned (`sylow_hip_fr_ntt_batch_tuned`): 1..=10, negative = the default.  The values do not depend on it.
pub fn fr_ntt_tuned(dev: &Device, a: &KzgPolys, inverse: bool, shift: Option<&Fr>, stages: i32) -> Result<KzgPolys, HipError> {
    let log_n = radix2_log(a.len);
    let dsh = match shift {
        Some(g) => Some(dev.upload_soa::<4>(&fr_words(std::slice::from_ref(g)))?),
        None => None,
    };
    let psh = dsh.as_ref().map_or(std::ptr::null(), |d| d.as_ptr());
    let out = dev.alloc::<u64>(4 * (1 << log_n) * a.m)?;
    // SAFETY: as fr_ntt.
    device::check(unsafe { ffi::sylow_hip_fr_ntt_batch_tuned(a.words.as_ptr(), log_n, a.m, inverse as i32, psh, stages, out.as_mut_ptr(), dev.stream) })?;
    Ok(KzgPolys { words: out, len: a.len, m: a.m })
}
/// m arrays of n = 2^log_n affine G1 points on the device as the G1 transform takes them: word w of point k of array j at (j * 8 + w) * n + k,
/// flags [m][n].  With m = 1 this is the layout of `DeviceG1`.
pub struct G1Arrays {
    pub xy: DeviceBuf<u64>,
    pub inf: DeviceBuf<u8>,
    pub n: usize,
    pub m: usize,
}
impl G1Arrays {
    /// one array: the points as they lie
    pub fn from_one(p: DeviceG1) -> Self {
        G1Arrays { n: p.n, m: 1, xy: p.xy, inf: p.inf }
    }
    /// the only array of a batch of one
    pub fn into_one(self) -> DeviceG1 {
        assert!(self.m == 1, "a batch of one array");
        DeviceG1 { n: self.n, xy: self.xy, inf: self.inf }
    }
}
/// The transform of `fr_ntt` with G1 POINTS as elements (`sylow_hip_g1_ntt_batch`), natural order in and out: forward
/// out_i = sum_k w_n^(ik) P_k, inverse out_k = n^-1 sum_i w_n^(-ik) P_i; no coset shift.  Points are taken as given; a flagged point, or the
/// pair (0, 1), is the identity.  Canonical affine words and flags out, in buffers of their own.
pub fn g1_ntt(dev: &Device, p: &G1Arrays, inverse: bool) -> Result<G1Arrays, HipError> {
    let log_n = radix2_log(p.n);
    let out = G1Arrays { xy: dev.alloc::<u64>(8 * (1 << log_n) * p.m)?, inf: dev.alloc::<u8>((1 << log_n) * p.m)?, n: p.n, m: p.m };
    // SAFETY: m arrays of 2^log_n points and their flags in and out (distinct buffers).
    device::check(unsafe {
        ffi::sylow_hip_g1_ntt_batch(p.xy.as_ptr(), p.inf.as_ptr(), log_n, p.m, inverse as i32, out.xy.as_mut_ptr(), out.inf.as_mut_ptr(), dev.stream)
    })?;
    Ok(out)
}
/// The same with the blocks of a stage launch capped (`sylow_hip_g1_ntt_batch_tuned`): >= 1, negative = the default; 0 is refused.  The points
/// do not depend on it.
pub fn g1_ntt_tuned(dev: &Device, p: &G1Arrays, inverse: bool, max_blocks: i64) -> Result<G1Arrays, HipError> {
    let log_n = radix2_log(p.n);
    let out = G1Arrays { xy: dev.alloc::<u64>(8 * (1 << log_n) * p.m)?, inf: dev.alloc::<u8>((1 << log_n) * p.m)?, n: p.n, m: p.m };
    // SAFETY: as g1_ntt.
    device::check(unsafe {
        ffi::sylow_hip_g1_ntt_batch_tuned(p.xy.as_ptr(), p.inf.as_ptr(), log_n, p.m, inverse as i32, max_blocks, out.xy.as_mut_ptr(), out.inf.as_mut_ptr(),
                                          dev.stream)
    })?;
    Ok(out)
}
/// The Lagrange-basis SRS L_i(tau) G1gen from the monomial one (`sylow_hip_kzg_srs_lagrange`): what `kzg_open_evals` takes.  A set flag in
/// the result means that tau lies in the domain and the SRS is unusable; the caller checks `inf`.
pub fn kzg_srs_lagrange(dev: &Device, srs: &DeviceG1) -> Result<DeviceG1, HipError> {
    let log_n = radix2_log(srs.n);
    let out = DeviceG1 { xy: dev.alloc::<u64>(8 * (1 << log_n))?, inf: dev.alloc::<u8>(1 << log_n)?, n: srs.n };
    // SAFETY: 2^log_n SRS points (no flags) in, as many points and flags out (distinct buffers).
    device::check(unsafe { ffi::sylow_hip_kzg_srs_lagrange(srs.xy.as_ptr(), log_n, out.xy.as_mut_ptr(), out.inf.as_mut_ptr(), dev.stream) })?;
    Ok(out)
}
/// The table of `kzg_open_all` from the monomial SRS of `srs.n` = 2^log_n <= 2^27 points (`sylow_hip_kzg_open_all_prepare`): the forward
/// G1 transform of 2n points, x_(2n-1-t) = s_t for t <= n - 2 and the identity elsewhere.  Once per SRS; a set flag is an entry that is
/// the identity, not an error.
pub fn kzg_open_all_prepare(dev: &Device, srs: &DeviceG1) -> Result<DeviceG1, HipError> {
    let log_n = open_all_log(srs.n);
    let table = DeviceG1 { xy: dev.alloc::<u64>(16 * (1 << log_n))?, inf: dev.alloc::<u8>(2 * (1 << log_n))?, n: 2 * srs.n };
    // SAFETY: 2^log_n SRS points (no flags) in, twice as many points and flags out (distinct buffers).
    device::check(unsafe { ffi::sylow_hip_kzg_open_all_prepare(srs.xy.as_ptr(), log_n, table.xy.as_mut_ptr(), table.inf.as_mut_ptr(), dev.stream) })?;
    Ok(table)
}
/// log2 of a domain `kzg_open_all` serves: the transform of twice as many points must fit the 2^28 roots
fn open_all_log(n: usize) -> i32 {
    assert!(n.is_power_of_two() && n <= 1 << 27, "a radix-2 domain of at most 2^27 points");
    n.trailing_zeros() as i32
}
/// The proofs of every f_j at ALL n = `p.len` = 2^log_n points w_n^i of its domain, in n log n, and its values there
/// (`sylow_hip_kzg_open_all_batch`): (y in the layout of `p`, y_ji = f_j(w^i); pi as m arrays of n points).  pi_ji is word for word what
/// `kzg_open` yields for f_j at w^i; `table` is what `kzg_open_all_prepare` returned for the SRS.
pub fn kzg_open_all(dev: &Device, table: &DeviceG1, p: &KzgPolys) -> Result<(KzgPolys, G1Arrays), HipError> {
    kzg_open_all_tuned(dev, table, p, -1)
}
/// The same with the blocks of a multiplying launch capped (`sylow_hip_kzg_open_all_batch_tuned`): >= 1, negative = the default; 0 is
/// refused.  The values do not depend on it.
pub fn kzg_open_all_tuned(dev: &Device, table: &DeviceG1, p: &KzgPolys, max_blocks: i64) -> Result<(KzgPolys, G1Arrays), HipError> {
    let log_n = open_all_log(p.len);
    assert!(table.n == 2 * p.len, "the table holds two entries per coefficient");
    let y = dev.alloc::<u64>(4 * (1 << log_n) * p.m)?;
    let pi = G1Arrays { xy: dev.alloc::<u64>(8 * (1 << log_n) * p.m)?, inf: dev.alloc::<u8>((1 << log_n) * p.m)?, n: p.len, m: p.m };
    // SAFETY: 2 * 2^log_n table entries and their flags, m arrays of 2^log_n coefficients in, as many values, points and flags out (distinct buffers).
    device::check(unsafe {
        if max_blocks < 0 {
            ffi::sylow_hip_kzg_open_all_batch(table.xy.as_ptr(), table.inf.as_ptr(), p.words.as_ptr(), log_n, p.m, y.as_mut_ptr(), pi.xy.as_mut_ptr(),
                                              pi.inf.as_mut_ptr(), dev.stream)
        } else {
            ffi::sylow_hip_kzg_open_all_batch_tuned(table.xy.as_ptr(), table.inf.as_ptr(), p.words.as_ptr(), log_n, p.m, max_blocks, y.as_mut_ptr(),
                                                    pi.xy.as_mut_ptr(), pi.inf.as_mut_ptr(), dev.stream)
        }
    })?;
    Ok((KzgPolys { words: y, len: p.len, m: p.m }, pi))
}
/// A sparse matrix over Fr on the device, in CSR: `row_ptr` [rows + 1], `col` [nnz], `val` [4][nnz].
pub struct CsrMatrix {
    pub row_ptr: DeviceBuf<u64>,
    pub col: DeviceBuf<u64>,
    pub val: DeviceBuf<u64>,
    pub rows: usize,
    pub nnz: usize,
}
impl CsrMatrix {
    /// `rows[i]` = the (column, value) entries of row i
    pub fn upload(dev: &Device, rows: &[Vec<(u64, Fr)>]) -> Result<Self, HipError> {
        let mut row_ptr = vec![0u64];
        let (mut col, mut val) = (Vec::new(), Vec::new());
        for row in rows {
            for (c, v) in row {
                col.push(*c);
                val.push(*v);
            }
            row_ptr.push(col.len() as u64);
        }
        let nnz = col.len();
        Ok(CsrMatrix { row_ptr: dev.upload(&row_ptr)?, col: dev.upload(&col)?, val: dev.upload_soa::<4>(&fr_words(&val))?, rows: rows.len(), nnz })
    }
}
/// out_j = M w_j over Fr for m vectors `w` of n_cols elements in the layout of `KzgPolys`, padded with zero rows to `n_out` >= M.rows
/// (`sylow_hip_fr_spmv_batch`).  An entry whose column is n_cols or more contributes zero; no read leaves the arrays.
pub fn fr_spmv(dev: &Device, mat: &CsrMatrix, w: &KzgPolys, n_out: usize) -> Result<KzgPolys, HipError> {
    assert!(n_out >= mat.rows && n_out >= 1);
    let (n_cols, m) = (w.len, w.m);
    let out = dev.alloc::<u64>(4 * n_out * m)?;
    // SAFETY: rows + 1 offsets, nnz columns and values, m vectors of n_cols elements, m arrays of n_out elements out.
    device::check(unsafe {
        ffi::sylow_hip_fr_spmv_batch(mat.row_ptr.as_ptr(), mat.col.as_ptr(), mat.val.as_ptr(), mat.rows, mat.nnz, w.words.as_ptr(), n_cols, m, n_out, out.as_mut_ptr(), dev.stream)
    })?;
    Ok(KzgPolys { words: out, len: n_out, m })
}
/// The same with 2^lanes_log lanes per row pinned (`sylow_hip_fr_spmv_batch_tuned`): 0..=6, negative = the default.  The values do not depend on it.
pub fn fr_spmv_tuned(dev: &Device, mat: &CsrMatrix, w: &KzgPolys, n_out: usize, lanes_log: i32) -> Result<KzgPolys, HipError> {
    assert!(n_out >= mat.rows && n_out >= 1);
    let (n_cols, m) = (w.len, w.m);
    let out = dev.alloc::<u64>(4 * n_out * m)?;
    // SAFETY: as fr_spmv.
    device::check(unsafe {
        ffi::sylow_hip_fr_spmv_batch_tuned(mat.row_ptr.as_ptr(), mat.col.as_ptr(), mat.val.as_ptr(), mat.rows, mat.nnz, w.words.as_ptr(), n_cols, m, n_out, lanes_log, out.as_mut_ptr(), dev.stream)
    })?;
    Ok(KzgPolys { words: out, len: n_out, m })
}
/// h = the coefficients of the polynomial of degree < n that equals (a b - c) / (X^n - 1) on the coset 5 <w_n>, for the values a, b, c of three
/// polynomials on the domain of n = 2^log_n points, m arrays each (`sylow_hip_groth16_quotient_batch`); h[n - 1] = 0 where a_i b_i = c_i everywhere.
pub fn groth16_quotient(dev: &Device, a: &KzgPolys, b: &KzgPolys, c: &KzgPolys) -> Result<KzgPolys, HipError> {
    assert!(a.len == b.len && a.len == c.len && a.m == b.m && a.m == c.m);
    let log_n = radix2_log(a.len);
    let h = dev.alloc::<u64>(4 * (1 << log_n) * a.m)?;
    // SAFETY: m arrays of 2^log_n elements each in a, b, c and out.
    device::check(unsafe { ffi::sylow_hip_groth16_quotient_batch(a.words.as_ptr(), b.words.as_ptr(), c.words.as_ptr(), log_n, a.m, h.as_mut_ptr(), dev.stream) })?;
    Ok(KzgPolys { words: h, len: a.len, m: a.m })
}
/// An R1CS for the prover: the CSR matrices a, b, c (n_cons rows, n_vars columns each); variable 0 is the constant 1, variables
/// 1..=n_inputs are public; the domain has 2^log_n >= n_cons points.
pub struct Groth16Circuit {
    pub a: CsrMatrix,
    pub b: CsrMatrix,
    pub c: CsrMatrix,
    pub n_vars: usize,
    pub n_inputs: usize,
    pub log_n: i32,
}
/// A Groth16 proving key on the device, arkworks' names: a_query, b_g1_query, b_g2_query hold n_vars points, h_query 2^log_n - 1,
/// l_query n_vars - n_inputs - 1; a query entry may be flagged as the identity.
pub struct Groth16Pk {
    pub alpha_g1: DeviceG1,
    pub beta_g1: DeviceG1,
    pub delta_g1: DeviceG1,
    pub beta_g2: DeviceG2,
    pub delta_g2: DeviceG2,
    pub a_query: DeviceG1,
    pub b_g1_query: DeviceG1,
    pub b_g2_query: DeviceG2,
    pub h_query: DeviceG1,
    pub l_query: DeviceG1,
}
/// m proofs (A, B, C) for the witnesses `z` (m arrays of n_vars elements) under one key with the caller's randomness r, s
/// (`sylow_hip_groth16_prove_batch`): what `groth16_verify` takes.  Neither z_0 = 1 nor the constraints are checked.
pub fn groth16_prove(dev: &Device, pk: &Groth16Pk, ct: &Groth16Circuit, z: &KzgPolys, r: &[Fr], s: &[Fr]) -> Result<(DeviceG1, DeviceG2, DeviceG1), HipError> {
    let m = z.m;
    assert!(z.len == ct.n_vars && r.len() == m && s.len() == m && ct.n_inputs < ct.n_vars);
    assert!(ct.a.rows == ct.b.rows && ct.a.rows == ct.c.rows && ct.a.rows <= 1 << ct.log_n);
    assert!(pk.alpha_g1.n == 1 && pk.beta_g1.n == 1 && pk.delta_g1.n == 1 && pk.beta_g2.n == 1 && pk.delta_g2.n == 1);
    assert!(pk.a_query.n == ct.n_vars && pk.b_g1_query.n == ct.n_vars && pk.b_g2_query.n == ct.n_vars);
    assert!(pk.h_query.n == (1 << ct.log_n) - 1 && pk.l_query.n == ct.n_vars - ct.n_inputs - 1);
    let (dr, ds) = (dev.upload_soa::<4>(&fr_words(r))?, dev.upload_soa::<4>(&fr_words(s))?);
    let a = DeviceG1 { xy: dev.alloc::<u64>(8 * m)?, inf: dev.alloc::<u8>(m)?, n: m };
    let b = DeviceG2 { xy: dev.alloc::<u64>(16 * m)?, inf: dev.alloc::<u8>(m)?, n: m };
    let c = DeviceG1 { xy: dev.alloc::<u64>(8 * m)?, inf: dev.alloc::<u8>(m)?, n: m };
    // SAFETY: three CSR matrices of n_cons rows, the key's arrays of the lengths asserted above, m witnesses, 4 * m words of r and of s,
    // m points and flags out for each of A, B, C.
    device::check(unsafe {
        ffi::sylow_hip_groth16_prove_batch(ct.a.row_ptr.as_ptr(), ct.a.col.as_ptr(), ct.a.val.as_ptr(), ct.a.nnz, ct.b.row_ptr.as_ptr(), ct.b.col.as_ptr(), ct.b.val.as_ptr(), ct.b.nnz,
            ct.c.row_ptr.as_ptr(), ct.c.col.as_ptr(), ct.c.val.as_ptr(), ct.c.nnz, ct.a.rows, ct.n_vars, ct.n_inputs, ct.log_n,
            pk.alpha_g1.xy.as_ptr(), pk.beta_g1.xy.as_ptr(), pk.delta_g1.xy.as_ptr(), pk.beta_g2.xy.as_ptr(), pk.delta_g2.xy.as_ptr(),
            pk.a_query.xy.as_ptr(), pk.a_query.inf.as_ptr(), pk.b_g1_query.xy.as_ptr(), pk.b_g1_query.inf.as_ptr(), pk.b_g2_query.xy.as_ptr(), pk.b_g2_query.inf.as_ptr(),
            pk.h_query.xy.as_ptr(), pk.h_query.inf.as_ptr(), pk.l_query.xy.as_ptr(), pk.l_query.inf.as_ptr(), z.words.as_ptr(), dr.as_ptr(), ds.as_ptr(), m,
            a.xy.as_mut_ptr(), a.inf.as_mut_ptr(), b.xy.as_mut_ptr(), b.inf.as_mut_ptr(), c.xy.as_mut_ptr(), c.inf.as_mut_ptr(), dev.stream)
    })?;
    Ok((a, b, c))
}
/// AND of a device-resident flag vector (one rank; `all_valid` in lib.rs adds the reduce over ranks).
pub fn flags_all(dev: &Device, flags: &DeviceBuf<u8>) -> Result<bool, HipError> {
    let out = dev.alloc::<i32>(1)?;
    // SAFETY: flags.len bytes, one int32 out.
    device::check(unsafe { ffi::sylow_hip_flags_all(flags.as_ptr(), flags.len, out.as_mut_ptr(), dev.stream) })?;
    Ok(dev.download(&out)?[0] == 1)
}
/// One signer, many messages, the key's line table rebuilt inside the call (examples/verify_multiple_messages_same_signer.rs:41-60);
/// `KeyTable` in lib.rs is the cached form.  `fused = true` names the one-final-exponentiation kernel explicitly.
pub fn verify_same_signer_batch(dev: &Device, pk: &G2Affine, msgs: &[&[u8]], sig: &[G1Affine]) -> Result<Vec<bool>, HipError> {
    assert_eq!(msgs.len(), sig.len());
    let n = msgs.len();
    let (dpk, dsig) = (upload_g2(dev, std::slice::from_ref(pk))?, upload_g1(dev, sig)?);
    let (d_msgs, d_off) = messages(dev, msgs)?;
    let ok = dev.alloc::<u8>(n)?;
    // SAFETY: one key, n signatures, n + 1 offsets, n flags.
    device::check(unsafe {
        ffi::sylow_hip_bls_verify_same_signer_batch(dpk.xy.as_ptr(), dpk.inf.as_ptr(), d_msgs.as_ptr(), d_off.as_ptr(), dsig.xy.as_ptr(), dsig.inf.as_ptr(),
                                                    ok.as_mut_ptr(), n, dev.stream)
    })?;
    Ok(dev.download(&ok)?.iter().map(|&f| f != 0).collect())
}
pub fn verify_fused_batch(dev: &Device, pk: &DeviceG2, msgs: &[&[u8]], sig: &DeviceG1) -> Result<Vec<bool>, HipError> {
    assert!(pk.n == msgs.len() && sig.n == msgs.len());
    let n = msgs.len();
    let (d_msgs, d_off) = messages(dev, msgs)?;
    let ok = dev.alloc::<u8>(n)?;
    // SAFETY: n keys, n signatures, n + 1 offsets, n flags.
    device::check(unsafe {
        ffi::sylow_hip_bls_verify_fused_batch(pk.xy.as_ptr(), pk.inf.as_ptr(), d_msgs.as_ptr(), d_off.as_ptr(), sig.xy.as_ptr(), sig.inf.as_ptr(), ok.as_mut_ptr(), n, dev.stream)
    })?;
    Ok(dev.download(&ok)?.iter().map(|&f| f != 0).collect())
}

// ------------------------------------------------------------------ examples/reth_bn128.rs: the EVM precompile adapters
pub mod evm {
    //! `run_add` / `run_mul` / `run_pair` (examples/reth_bn128.rs:99-217) as batches over the precompiles' byte formats.  Inputs are
    //! padded / truncated by the caller exactly as the reference's `right_pad` does; per-job status bytes mirror `GroupError`.
    use super::*;

    /// n x 128 bytes (two G1 points) -> n x 64 bytes + status.
    pub fn run_add(dev: &Device, input: &[[u8; 128]]) -> Result<(Vec<[u8; 64]>, Vec<u8>), HipError> {
        let n = input.len();
        let flat: Vec<u8> = input.iter().flatten().copied().collect();
        let (d_in, out, st) = (dev.upload(&flat)?, dev.alloc::<u8>(64 * n)?, dev.alloc::<u8>(n)?);
        // SAFETY: 128 * n bytes in, 64 * n bytes and n status bytes out.
        device::check(unsafe { ffi::sylow_hip_evm_ecadd_batch(d_in.as_ptr(), out.as_mut_ptr(), st.as_mut_ptr(), n, dev.stream) })?;
        Ok((dev.download(&out)?.chunks_exact(64).map(|c| c.try_into().unwrap()).collect(), dev.download(&st)?))
    }
    /// n x 96 bytes (a G1 point and a 256-bit scalar, reduced mod r as EIP-196 requires) -> n x 64 bytes + status.
    pub fn run_mul(dev: &Device, input: &[[u8; 96]]) -> Result<(Vec<[u8; 64]>, Vec<u8>), HipError> {
        let n = input.len();
        let flat: Vec<u8> = input.iter().flatten().copied().collect();
        let (d_in, out, st) = (dev.upload(&flat)?, dev.alloc::<u8>(64 * n)?, dev.alloc::<u8>(n)?);
        // SAFETY: 96 * n bytes in, 64 * n bytes and n status bytes out.
        device::check(unsafe { ffi::sylow_hip_evm_ecmul_batch(d_in.as_ptr(), out.as_mut_ptr(), st.as_mut_ptr(), n, dev.stream) })?;
        Ok((dev.download(&out)?.chunks_exact(64).map(|c| c.try_into().unwrap()).collect(), dev.download(&st)?))
    }
    /// Jobs of k_j pairs of 192 bytes each (`jobs[j].len() == 192 * k_j`) -> (pairing check result, status) per job.
    pub fn run_pair(dev: &Device, jobs: &[&[u8]]) -> Result<(Vec<bool>, Vec<u8>), HipError> {
        let n_jobs = jobs.len();
        let mut offsets = Vec::with_capacity(n_jobs + 1);
        let mut flat = Vec::new();
        offsets.push(0u64);
        for j in jobs {
            assert_eq!(j.len() % 192, 0);
            flat.extend_from_slice(j);
            offsets.push((flat.len() / 192) as u64);
        }
        let n_pairs = flat.len() / 192;
        if flat.is_empty() {
            flat.push(0);
        }
        let (d_in, d_off) = (dev.upload(&flat)?, dev.upload(&offsets)?);
        let (res, st) = (dev.alloc::<u8>(n_jobs.max(1))?, dev.alloc::<u8>(n_jobs.max(1))?);
        // SAFETY: 192 * n_pairs bytes, n_jobs + 1 offsets, n_jobs result and status bytes.
        device::check(unsafe { ffi::sylow_hip_evm_ecpairing_batch(d_in.as_ptr(), d_off.as_ptr(), n_jobs, n_pairs, res.as_mut_ptr(), st.as_mut_ptr(), dev.stream) })?;
        Ok((dev.download(&res)?[..n_jobs].iter().map(|&f| f != 0).collect(), dev.download(&st)?[..n_jobs].to_vec()))
    }
}

// ------------------------------------------------------------------ process-level plumbing
/// Number of GPUs the library can see, and `sylow_hip_init_devices` for hosts that drive several GPUs from one process.
pub fn device_count() -> i32 {
    // SAFETY: no arguments.
    unsafe { ffi::sylow_hip_device_count() }
}
pub fn init_devices(ordinals: &[i32]) -> Result<(), device::Error> {
    // SAFETY: a host array of ordinals.len() int32.
    device::check(unsafe { ffi::sylow_hip_init_devices(ordinals.as_ptr(), ordinals.len() as i32) })
}
/// The seeded xoshiro256** stream of BASELINE.md §3 (bench and test inputs; NOT a cryptographic generator): n draws below p.
pub fn xoshiro_fp(seed: u64, n: usize) -> Result<Vec<Fp>, device::Error> {
    let mut soa = vec![0u64; 4 * n];
    // SAFETY: a HOST array in the library's SoA layout [4][stride] with stride = n.
    device::check(unsafe { ffi::sylow_hip_host_xoshiro_fp(seed, soa.as_mut_ptr(), n, n) })?;
    Ok((0..n).map(|i| fp_from_words(&[soa[i], soa[n + i], soa[2 * n + i], soa[3 * n + i]])).collect())
}

// ------------------------------------------------------------------ host-array pipelines on canonical words
/// Page-locked host memory (`sylow_hip_host_malloc`): staging arrays for the `*_host` calls, whose copies then run asynchronously
/// beside the kernels.  Freed on drop.
pub struct PinnedBuf<T: Copy> {
    ptr: *mut T,
    len: usize,
}
impl<T: Copy> PinnedBuf<T> {
    pub fn new(len: usize) -> Result<Self, device::Error> {
        let mut p: *mut c_void = std::ptr::null_mut();
        // SAFETY: `p` is a valid out-pointer.
        device::check(unsafe { ffi::sylow_hip_host_malloc(&mut p, len * std::mem::size_of::<T>()) })?;
        Ok(PinnedBuf { ptr: p as *mut T, len })
    }
    pub fn as_slice(&self) -> &[T] {
        // SAFETY: `len` elements were allocated; T: Copy has no drop glue and every bit pattern written by the library is a valid integer.
        unsafe { std::slice::from_raw_parts(self.ptr, self.len) }
    }
    pub fn as_mut_slice(&mut self) -> &mut [T] {
        // SAFETY: as above; unique borrow.
        unsafe { std::slice::from_raw_parts_mut(self.ptr, self.len) }
    }
}
impl<T: Copy> Drop for PinnedBuf<T> {
    fn drop(&mut self) {
        // SAFETY: the pointer came from sylow_hip_host_malloc.
        unsafe { ffi::sylow_hip_host_free(self.ptr as *mut c_void) };
    }
}

/// `pairing` on canonical words held by the host (x, y per G1 point: `[u64; 8]`; x.c0, x.c1, y.c0, y.c1 per G2 point: `[u64; 16]`):
/// the chunked two-stream pipeline of `sylow_hip_pairing_host`, writing into `gt` (which may live in a `PinnedBuf`).
pub fn pairing_words_host(p: &[[u64; 8]], p_inf: Option<&[u8]>, q: &[[u64; 16]], q_inf: Option<&[u8]>, gt: &mut [[u64; 48]]) -> Result<(), device::Error> {
    let n = p.len();
    assert!(q.len() == n && gt.len() == n && p_inf.map_or(true, |f| f.len() == n) && q_inf.map_or(true, |f| f.len() == n));
    // SAFETY: n elements in every array; host memory; the call returns after the last copy has landed.
    device::check(unsafe {
        ffi::sylow_hip_pairing_host(p.as_ptr() as *const u64, p_inf.map_or(std::ptr::null(), |f| f.as_ptr()), q.as_ptr() as *const u64,
                                    q_inf.map_or(std::ptr::null(), |f| f.as_ptr()), gt.as_mut_ptr() as *mut u64, n, 0)
    })
}

/// `verify` on canonical words held by the host (`sylow_hip_bls_verify_host`): ok[i] = verify(pk[i], msgs[offsets[i]..offsets[i + 1]], sig[i]).
pub fn verify_words_host(pk: &[[u64; 16]], pk_inf: Option<&[u8]>, msgs: &[u8], offsets: &[u64], sig: &[[u64; 8]], sig_inf: Option<&[u8]>,
                         ok: &mut [u8]) -> Result<(), device::Error> {
    let n = pk.len();
    assert!(sig.len() == n && ok.len() == n && offsets.len() == n + 1 && *offsets.last().unwrap() as usize <= msgs.len());
    assert!(pk_inf.map_or(true, |f| f.len() == n) && sig_inf.map_or(true, |f| f.len() == n));
    // SAFETY: n keys / signatures / flags, n + 1 offsets into msgs; host memory; synchronous call.
    device::check(unsafe {
        ffi::sylow_hip_bls_verify_host(pk.as_ptr() as *const u64, pk_inf.map_or(std::ptr::null(), |f| f.as_ptr()), msgs.as_ptr(), offsets.as_ptr(),
                                       sig.as_ptr() as *const u64, sig_inf.map_or(std::ptr::null(), |f| f.as_ptr()), ok.as_mut_ptr(), n, 0)
    })
}

/// sum_i p[i] as one point (`sylow_hip_g1_sum_batch`): the `+` fold of examples/verify_multiple_messages_same_signer.rs:41-60 over a resident batch.
pub fn g1_sum(dev: &Device, p: &DeviceG1) -> Result<G1Projective, HipError> {
    let out = DeviceG1 { xy: dev.alloc::<u64>(8)?, inf: dev.alloc::<u8>(1)?, n: 1 };
    // SAFETY: p holds p.n points and flags; out one point and one flag.
    device::check(unsafe { ffi::sylow_hip_g1_sum_batch(p.xy.as_ptr(), p.inf.as_ptr(), p.n, out.xy.as_mut_ptr(), out.inf.as_mut_ptr(), dev.stream) })?;
    Ok(download_g1(dev, &out)?.remove(0))
}

/// sum_i q[i] as one G2 point (`sylow_hip_g2_sum_batch`): the `+` fold of examples/dkg.rs:309-314 over a resident batch of public keys.
pub fn g2_sum(dev: &Device, q: &DeviceG2) -> Result<DeviceG2, HipError> {
    let out = DeviceG2 { xy: dev.alloc::<u64>(16)?, inf: dev.alloc::<u8>(1)?, n: 1 };
    // SAFETY: q holds q.n points and flags; out one point and one flag.
    device::check(unsafe { ffi::sylow_hip_g2_sum_batch(q.xy.as_ptr(), q.inf.as_ptr(), q.n, out.xy.as_mut_ptr(), out.inf.as_mut_ptr(), dev.stream) })?;
    Ok(out)
}
/// n_jobs weighted sums sum_i k[j][i] * q[j][i] in G2 (`sylow_hip_g2_lincomb_batch`: a threshold group key sum_i lambda_i pk_i), term-major
/// input: element (job j, term i) at index i * n_jobs + j.  Scalars are Fp values and the products are exact on the whole twist.
pub fn g2_lincomb(dev: &Device, q: &DeviceG2, k: &[Fp], n_jobs: usize, n_terms: usize) -> Result<DeviceG2, HipError> {
    assert!(q.n == n_jobs * n_terms && k.len() == q.n);
    let dk = dev.upload_soa::<4>(&fp_words(k))?;
    let out = DeviceG2 { xy: dev.alloc::<u64>(16 * n_jobs)?, inf: dev.alloc::<u8>(n_jobs)?, n: n_jobs };
    // SAFETY: n_jobs * n_terms points and scalars, n_jobs outputs.
    device::check(unsafe {
        ffi::sylow_hip_g2_lincomb_batch(q.xy.as_ptr(), q.inf.as_ptr(), dk.as_ptr(), out.xy.as_mut_ptr(), out.inf.as_mut_ptr(), n_jobs, n_terms, dev.stream)
    })?;
    Ok(out)
}
/// sum_i k[i] * q[i] as one G2 point by the bucket method (`sylow_hip_g2_msm`: a rogue-key-safe aggregate key sum_i t_i pk_i, the G2 half of
/// a KZG verifier); the same point as `g2_lincomb(dev, q, k, 1, q.n)`.
pub fn g2_msm(dev: &Device, q: &DeviceG2, k: &[Fp]) -> Result<DeviceG2, HipError> {
    assert!(k.len() == q.n);
    let n = q.n;
    let dk = dev.upload_soa::<4>(&fp_words(k))?;
    let out = DeviceG2 { xy: dev.alloc::<u64>(16)?, inf: dev.alloc::<u8>(1)?, n: 1 };
    // SAFETY: n points and scalars (possibly empty), one output point.
    device::check(unsafe {
        ffi::sylow_hip_g2_msm(q.xy.as_ptr(), q.inf.as_ptr(), dk.as_ptr(), n, out.xy.as_mut_ptr(), out.inf.as_mut_ptr(), dev.stream)
    })?;
    Ok(out)
}
/// `g2_msm` with the plan pinned (`sylow_hip_g2_msm_tuned`): window width 4..16 and the smallest n on the bucket route; < 0 = the
/// defaults.  The point does not depend on either.
pub fn g2_msm_tuned(dev: &Device, q: &DeviceG2, k: &[Fp], window: i32, min_n: i64) -> Result<DeviceG2, HipError> {
    assert!(k.len() == q.n);
    let n = q.n;
    let dk = dev.upload_soa::<4>(&fp_words(k))?;
    let out = DeviceG2 { xy: dev.alloc::<u64>(16)?, inf: dev.alloc::<u8>(1)?, n: 1 };
    // SAFETY: n points and scalars (possibly empty), one output point.
    device::check(unsafe {
        ffi::sylow_hip_g2_msm_tuned(q.xy.as_ptr(), q.inf.as_ptr(), dk.as_ptr(), n, window, min_n, out.xy.as_mut_ptr(), out.inf.as_mut_ptr(), dev.stream)
    })?;
    Ok(out)
}

/// Upper bound for the line tables of the multi-pair routes (`sylow_hip_set_scratch_limit`; 0 = the default of 12 GB): the one scratch
/// user whose size is not proportional to its input.  Process-wide; results do not depend on it.
pub fn set_scratch_limit(bytes: usize) -> Result<(), device::Error> {
    // SAFETY: no pointers.
    device::check(unsafe { ffi::sylow_hip_set_scratch_limit(bytes) })
}

/// The library's route selectors and thresholds (`SYLOW_HIP_OPT_*` of include/sylow_hip.h; the library reads no environment variable).
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
#[repr(i32)]
pub enum RouteOption { Stagger = 0, MultiTables = 1, WideTail = 2, WidePack = 3, AggFork = 4, SignWideMax = 5, WideMax = 6, WideVerifyMax = 7, QuadMax = 8, TailSplit = 9 }

/// `sylow_hip_set_option`: `None` restores the default.  Process-wide; results do not depend on any setting.
pub fn set_option(option: RouteOption, value: Option<u64>) -> Result<(), device::Error> {
    // SAFETY: plain value arguments.
    device::check(unsafe { ffi::sylow_hip_set_option(option as i32, value.map_or(-1, |v| v as i64)) })
}

/// `sylow_hip_get_option`: `None` = the default is in force.
pub fn get_option(option: RouteOption) -> Result<Option<u64>, device::Error> {
    let mut v: i64 = -1;
    // SAFETY: one host word.
    device::check(unsafe { ffi::sylow_hip_get_option(option as i32, &mut v) })?;
    Ok(if v < 0 { None } else { Some(v as u64) })
}

/// Live clock probe of the metric's kernels (`sylow_hip_clock_probe`): `acc` = 256 zeroed device words, or `None` to switch it off.  The
/// buffer must outlive the probe.  Returns the accumulators' meaning in include/sylow_hip.h.
pub fn clock_probe(acc: Option<&DeviceBuf<u64>>) -> Result<(), device::Error> {
    if let Some(a) = acc { assert!(a.len >= 256); }
    // SAFETY: a device buffer of at least 256 words, or NULL.
    device::check(unsafe { ffi::sylow_hip_clock_probe(acc.map_or(ptr::null_mut(), |a| a.as_mut_ptr())) })
}

/// Rate of the constant-rate counter the clock probe reads, in kHz (`sylow_hip_wall_clock_khz`).
pub fn wall_clock_khz() -> Result<i32, device::Error> {
    let mut khz: i32 = 0;
    // SAFETY: one host word.
    device::check(unsafe { ffi::sylow_hip_wall_clock_khz(&mut khz) })?;
    Ok(khz)
}

/// Hand the current device's idle scratch blocks above `keep_bytes` back to the driver (`sylow_hip_trim`): the library keeps the largest
/// block a call has needed for reuse, which after a 2^20-pair product is several GB.
pub fn trim(keep_bytes: usize) -> Result<(), device::Error> {
    // SAFETY: plain value argument.
    device::check(unsafe { ffi::sylow_hip_trim(keep_bytes) })
}
