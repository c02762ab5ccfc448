// A made-up gadget file, written for tests/test_rust_shim.py: every construct tools/reference_api_surface.py has to count right.
// Calls in comments are not calls: cs.multiply(a, b, c) prover.commit(x)
use bulletproofs::r1cs::{ConstraintSystem, Prover, Verifier};

/* block comments too:
   verifier.commit(c1);
   Prover::new(&pc_gens, &mut transcript, extra);
*/
pub fn sample_gadget<CS: ConstraintSystem>(cs: &mut CS, v: Vec<u64>) -> Result<(), R1CSError> {
    let (a, b, o) = cs.multiply(v[0].into(), (v[1] - 1u64).into());
    cs.constrain(o - a);
    cs.constrain(v.iter().fold(o.into(), |acc, x| acc - Scalar::from(*x)));
    let (l, _, _) = cs.allocate_multiplier(v.iter().map(|x| Scalar::from(*x)).next());
    let s = cs.allocate_single(Some(f(1, 2)))?;
    let t = cs.evaluate_lc(&vec![(l, Scalar::one()), (b, Scalar::one())].into());
    other.multiply(a, b);
    Ok(())
}

fn sample_test() {
    let pc_gens = PedersenGens::default();
    let bp_gens = BulletproofGens::new(128, 1);
    let mut prover_transcript = Transcript::new(b"Sample");
    let mut prover = Prover::new(&pc_gens, &mut prover_transcript);
    let (com, var) = prover.commit(Scalar::from(7u64), Scalar::random(&mut rng));
    let proof = prover.prove(&bp_gens).unwrap();
    let mut verifier_transcript = Transcript::new(b"Sample");
    let mut verifier = Verifier::new(&mut verifier_transcript);
    let var = verifier.commit(com);
    assert!(verifier.verify(&proof, &pc_gens, &bp_gens).is_ok());
    let c = pc_gens.commit(Scalar::one(), Scalar::zero());
    let n = bp_gens.share(0).G(4).collect::<Vec<_>>();
    let v = verifier.verify::<u8>(&proof, &pc_gens, &bp_gens);
}
