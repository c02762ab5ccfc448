/* bpr1cs.h — C ABI of the MI355X-native Bulletproofs R1CS prover hot path.
 *
 * Drop-in boundary for lovesh/bulletproofs-r1cs-gadgets.  The reference has no
 * FFI: its gadgets are generic over the Rust trait `bulletproofs::r1cs::
 * ConstraintSystem` and the hot path sits behind `Prover::commit` /
 * `Prover::prove` (reference src/gadget_vsmt_4.rs:393,434).  A
 * patched `bulletproofs` crate (or this repo's C++ front-end, which mirrors the
 * trait) forwards to the entry points below — see INTEGRATION.md for the Rust
 * `extern "C"` binding.
 *
 * Conventions: all scalars and points are 32-byte little-endian canonical
 * encodings (Scalar::to_bytes / CompressedRistretto); all buffers are
 * caller-owned host memory unless a name ends in `_dev`; return 0 = OK,
 * negative = bpr1cs_error (mirrors R1CSError).  No exceptions cross the ABI.
 * Threading: a handle may be used from one thread at a time; distinct handles are
 * independent (two threads may prove / verify concurrently on two bpr1cs_gens handles,
 * sharing a bpr1cs_circuit); options belong to a handle (bpr1cs_gens_create_opts,
 * bpr1cs_gens_set_option) - the library has no process-wide settings that change what a call does (the environment is read
 * for diagnostics only, listed under "Environment" below).  bpr1cs_last_prove_stats
 * reports the last prove call that returned on the calling thread.  There is NO CPU fallback: every compute entry point fails with
 * BPR1CS_ERR_NO_DEVICE when no gfx950 device is visible.  Device failures (HIP errors,
 * out of memory) are reported as BPR1CS_ERR_DEVICE / BPR1CS_ERR_OUT_OF_MEMORY; the
 * library never aborts the process.  All scalar inputs must be canonical (< l);
 * non-canonical scalars are refused with BPR1CS_ERR_INVALID_ARGUMENT.
 *
 * TIMING SIDE CHANNELS - by default this library is NOT constant time; a handle created with BPR1CS_OPT_SECRET_INDEPENDENT = 1
 * gives the commit phase the property the reference's prover has for it.  Upstream computes the V's, A_I, A_O, S and the T's
 * (sums over the secret values, wires and blindings) with curve25519-dalek's constant-time code and the L_k / R_k of
 * the inner-product argument with `vartime_multiscalar_mul` (public after the fact).  With the option on, exactly those
 * quantities are computed by k_msm_fixed_ct, which reads whole table rows at wave-uniform addresses and selects by scan: no
 * address, branch, vote or grid of the commit phase depends on a secret.  Outside that contract in either mode, as upstream or
 * public: the inner-product rounds, the verifier, the witness program (it branches on committed bits, as the reference's gadget
 * code does on the host), the host front-end, compression of the resulting points.  Keccak / STROBE is data-independent.
 * BPR1CS_OPT_CHECK_WITNESS adds two kernels whose addresses and grids are functions of the circuit and the batch size; their one
 * value-dependent branch is "this multiplier / row sum is violated", never taken for a satisfied witness and, for a violated
 * one, revealed by the refusal record anyway.
 * With the option off (the default) every multiscalar multiplication runs through k_msm_fixed2, which (i) gathers table entries at addresses that are the signed digits of
 * the secret scalars (memory-access pattern = secret), (ii) skips a term when the scalars of all 64 proofs of a
 * wavefront are zero, and (iii) takes the a_O wires of Inverse-S-box triples in the form a_O - 1, so that a proof whose
 * S-box input is 0 (an unsatisfiable witness: is_nonzero fails) makes its wavefront do work the others skip.  The witness
 * kernel branches on committed bits.  Results are identical; only the time and the memory traffic depend on secrets.
 * This is the usual posture of a throughput prover on a device the prover owns (nobody else can observe its caches or
 * timing); do not run it where an untrusted party shares the GPU or can time individual batches of a victim's witnesses.
 * Secrets (wires, blindings, the blinding vectors, l / r and everything derived from them: product scalars, Straus digits,
 * partial inner products) are wiped from device memory before their blocks return to the allocator (upstream: clear_on_drop).
 * Memory: the allocator refuses a large block that would leave less than BPR1CS_MEM_RESERVE_MB (environment, default 1024) of
 * device memory free - the HIP runtime aborts the process when IT finds none - and reports BPR1CS_ERR_OUT_OF_MEMORY instead.
 *
 * Environment (everything the shipped library reads; none changes a result): BPR1CS_MEM_RESERVE_MB (above, read once),
 * BPR1CS_DEBUG_MEM (prints the free device memory after every large allocation), BPR1CS_DEBUG_SYNC (synchronises after every
 * launch - the functor kernels and the hand-written ones alike: all go through one launch function - so that a faulting kernel
 * is named),BPR1CS_WITNESS_MACRO=0 (bpr1cs_circuit_create ignores the joint-evaluation
 * annotations of Poseidon permutations: the witness program then runs S-box by S-box - slower, same wires).  Failure
 * injection and table-geometry overrides of the test suite exist in the CPU simulator build of the tests only.
 */
#ifndef BPR1CS_H
#define BPR1CS_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    BPR1CS_OK = 0,
    BPR1CS_ERR_INVALID_GENERATORS_LENGTH = -1, /* R1CSError::InvalidGeneratorsLength */
    BPR1CS_ERR_FORMAT = -2,                    /* R1CSError::FormatError            */
    BPR1CS_ERR_VERIFICATION = -3,              /* R1CSError::VerificationError      */
    BPR1CS_ERR_MISSING_ASSIGNMENT = -4,        /* R1CSError::MissingAssignment      */
    BPR1CS_ERR_GADGET = -5,                    /* R1CSError::GadgetError            */
    BPR1CS_ERR_NO_DEVICE = -16,
    BPR1CS_ERR_INVALID_ARGUMENT = -17,
    BPR1CS_ERR_DEVICE = -18,       /* a HIP call failed */
    BPR1CS_ERR_OUT_OF_MEMORY = -19 /* device (or host) memory exhausted, also after dropping the allocator cache */
} bpr1cs_error;

typedef struct bpr1cs_gens bpr1cs_gens;       /* PedersenGens::default() + BulletproofGens::new(cap, 1) */
typedef struct bpr1cs_circuit bpr1cs_circuit; /* the constraint system a Prover holds when prove() is called */

/* Variable encoding used in constraint terms: (kind << 28) | index. */
#define BPR1CS_VAR_COMMITTED 0u /* Variable::Committed(i)        */
#define BPR1CS_VAR_MUL_LEFT 1u  /* Variable::MultiplierLeft(i)   */
#define BPR1CS_VAR_MUL_RIGHT 2u /* Variable::MultiplierRight(i)  */
#define BPR1CS_VAR_MUL_OUT 3u   /* Variable::MultiplierOutput(i) */
#define BPR1CS_VAR_ONE 4u       /* Variable::One()               */
#define BPR1CS_VAR_PUBLIC 5u    /* public input k of THIS proof: a scalar the verifier knows (see "Public inputs" below) */
#define BPR1CS_VAR_SCALE 8u     /* not a term of its own: multiplies the coefficient of the term that FOLLOWS it in the same row /
                                   combination by (its own coefficient) x p_k, p_k = public input k of the proof at hand (see "Public
                                   coefficients" below).  (8 is free: the variable kinds pinned as refused are 6, 7, 9 and 10.) */

/* Public inputs.  A constant of the statement that differs from proof to proof - the root of the reference's tree gadgets
 * (`constrain(prev_hash - root)`, src/gadget_vsmt_4.rs, src/gadget_vsmt_2.rs), a bound - need not be baked into the coefficient of
 * Variable::One(): a term (BPR1CS_VAR_PUBLIC << 28 | k, coeff) in `term_var` or `lc_var` stands for coeff x p_k, p_k the k-th public
 * input of the proof at hand.  bpr1cs_circuit_create derives p = 1 + the highest index used (p <= 2^20; p = 0 when the kind does not
 * occur, and then every call is exactly what it was).  Only a term that uses its input may set p: a public term whose coefficient is
 * 0 (mod l) is BPR1CS_ERR_INVALID_ARGUMENT (leave the term out).  No entry point reports p: a caller derives it from its own
 * description by the same rule, and the library - which cannot see how long the caller's arrays are - reads exactly batch x p x 32
 * bytes behind the committed values / points.  A public input enters LINEARLY with a constant coefficient, like One;
 * BPR1CS_W_BIT / BPR1CS_W_NOTBIT of one are BPR1CS_ERR_INVALID_ARGUMENT.  A public COEFFICIENT of a wire (the set_i x bit_i of
 * gadget_set_membership.rs) is written with BPR1CS_VAR_SCALE ("Public coefficients" below).
 * The values ride in arrays the calls already take, as a tail block:
 *   prove calls   `values`      = batch x m x 32 committed values, then batch x p x 32 public inputs, proof-major
 *                 (v_blindings, commitments_out, transcripts: over the m committed values only, as before)
 *   verify calls  `commitments` = batch x m x 32 points, then batch x p x 32 canonical scalars, proof-major; non-NULL when p > 0
 * A non-canonical public input: BPR1CS_ERR_INVALID_ARGUMENT for the prover (like every scalar input); for the verifiers that proof
 * is malformed (verdict 0 / wellformed_out = 0) and the others are judged as always.  Public inputs are NOT appended to the proof's
 * Merlin transcript - upstream absorbs no constants either -, so a proof is byte for byte the proof of the circuit that has
 * coeff x p_k folded into its One coefficients, and a verifier running that baked circuit accepts it.  The cross-proof weights DO
 * bind them (bpr1cs_verify_batch_combined). */

/* Public coefficients.  A marker (BPR1CS_VAR_SCALE << 28 | k, s) followed, in the same row of `term_var` or the same combination of
 * `lc_var`, by a term (var, c) stands for the SINGLE term s c p_k x var: the coefficient of a wire or of a committed value differs
 * from proof to proof (a set whose items are per-proof data, a weighted sum with per-proof weights) without a multiplier per
 * coefficient.  `var` is of kind COMMITTED, MUL_LEFT, MUL_RIGHT or MUL_OUT, and every check of an unmarked term applies to it
 * unchanged (a combination reads wires of EARLIER multipliers only, a committed index is < m).  BPR1CS_ERR_INVALID_ARGUMENT: a marker
 * that is the last term of its row or combination; a marker followed by One, a public term or another marker; k >= 2^20; s or c
 * that is non-canonical or 0 (mod l) - as for public terms, only a term that uses its input may size p.  Combinations named by
 * BPR1CS_W_LC, BPR1CS_W_LCBIT / BPR1CS_W_LCNOTBIT and Poseidon annotations may all hold marked terms.
 * NOT provided: a public input times One - that is BPR1CS_VAR_PUBLIC, which stays the only way to write it - and products of two
 * public inputs.
 * p = 1 + the highest index over public terms AND markers, in rows and combinations.  The values ride where they ride today - the
 * tail block of `values` and of `commitments` - and no call signature changes.  A description without a marker is byte for byte
 * what it was, creates the same circuit object and launches the same kernels.
 * Public inputs stay out of the Merlin transcript, so a proof is byte for byte the proof of the circuit with s c p_k baked in as a
 * constant coefficient, and a verifier running that baked circuit accepts it.  The cross-proof weights already absorb all p public
 * inputs of a proof (bpr1cs_verify_batch_combined), whichever way the circuit uses them: nothing changes there. */

/* Witness-program operand kinds (device-side constraint synthesis). */
#define BPR1CS_W_LC 0u       /* value of linear combination #arg (cs.multiply / evaluate_lc)   */
#define BPR1CS_W_INV_LEFT 1u /* right wire = inverse of this multiplier's left wire (Inverse S-box, gadget_poseidon.rs:160-166) */
#define BPR1CS_W_BIT 2u      /* bit (arg & 0xff) of committed value (arg >> 8)  (gadget_vsmt_4.rs:226-238, r1cs_utils.rs:28-31) */
#define BPR1CS_W_NOTBIT 3u   /* 1 - that bit */
#define BPR1CS_W_LCBIT 4u    /* bit (arg & 0xff) of the canonical value x, 0 <= x < l, of linear combination #(arg >> 8) */
#define BPR1CS_W_LCNOTBIT 5u /* 1 - that bit */
#define BPR1CS_W_AUX 10u     /* auxiliary input #arg of THIS proof: a wire the prover chooses freely (see "Auxiliary inputs" below); operand
                                kinds 6 .. 9 are not part of the ABI and stay BPR1CS_ERR_INVALID_ARGUMENT, as they always were */
/* Auxiliary inputs.  A wire the prover assigns without deriving it from anything - upstream's `cs.allocate(Some(x))` and
 * `allocate_multiplier(Some((l, r)))`: the nodes of a Merkle path, which link to nothing outside the proof - need not be a Pedersen
 * commitment for the device program to know it: an operand (BPR1CS_W_AUX, k) stands for a_k, the k-th auxiliary input of the proof at
 * hand.  Either side of any multiplier may be one; BPR1CS_W_INV_LEFT on the right of a BPR1CS_W_AUX left is allowed.  It is an OPERAND
 * kind only: linear combinations and bit operands reach the value through the wire it was written to (wires of EARLIER multipliers,
 * as always), and a variable of kind 6 or above in `term_var` or `lc_var` stays BPR1CS_ERR_INVALID_ARGUMENT - an auxiliary value is not a variable.
 * bpr1cs_circuit_create derives a = 1 + the highest index the operands of `wops` name (a <= 2^20: an index >= 2^20 is
 * BPR1CS_ERR_INVALID_ARGUMENT; a = 0 when the kind does not occur or the description has no `wops`, and then every call is exactly
 * what it was).  Indices below a that no operand names are allowed - the caller still supplies them - and several operands may name
 * one index.  No entry point reports a: a caller derives it from its own description by the same rule.
 * The values ride in the array the prove calls already take, as one more tail block:
 *   prove calls   `values`      = batch x m x 32 committed values, then batch x p x 32 public inputs, then batch x a x 32 auxiliary
 *                 inputs, proof-major, canonical  (bpr1cs_prove_batch, _transcripts, _draws, _begin; v_blindings, commitments_out,
 *                 transcripts: over the m committed values only, as before)
 * The block is read only when the device program runs (wires == NULL): with host wires it is not read and may be absent.  a > 0 with
 * wires == NULL and values == NULL, and a non-canonical auxiliary scalar, are BPR1CS_ERR_INVALID_ARGUMENT (like every scalar input of
 * the prover).  The verify calls never see the block: the verifier allocates the wire and learns nothing of its value.  Auxiliary
 * inputs are secrets and are wiped wherever committed values are. */
/* BPR1CS_W_LCBIT / BPR1CS_W_LCNOTBIT give the bits of a DERIVED value - v - min, a product wire, a hash output, v - Public(0) - so that
 * a range check needs no commitment beside v.  Either may be a left or a right operand.  The combination index is < n_lc (and < 2^24:
 * it shares `arg` with the bit index); the combination may read what a BPR1CS_W_LC operand of the same multiplier may read - committed
 * values, One, public inputs, wires of EARLIER multipliers - and BPR1CS_ERR_INVALID_ARGUMENT is returned for an index >= n_lc and for a
 * combination that reads the multiplier's own or a later wire, as for BPR1CS_W_LC.  l < 2^253: bits 253..255 are always 0 (NOTBIT: 1).
 * A combination only these kinds refer to counts towards p like any other.  The value is evaluated once per run of operands that
 * name the same combination (a k-bit decomposition names it 2k times in a row), so list the bits of one value together.  A
 * description that uses neither kind is byte for byte what it was.
 * BPR1CS_W_INV_LEFT of a left wire of 0 yields 0 (Scalar::invert's ladder does the same; safegcd: 0 -> 0), so the multiplier's
 * output is 0 where the left wire is 0 and 1 elsewhere: the witness of an "is zero" test on a derived value. */

typedef struct {
    uint32_t lkind, larg, rkind, rarg;
} bpr1cs_wop;

/* Optional annotation of a witness program: a Poseidon permutation with the Inverse S-box
 * (Poseidon_permutation_constraints, gadget_poseidon.rs:282-399, SboxType::Inverse :153-185).  The program stays
 * complete without it (every S-box multiplier carries BPR1CS_W_LC / BPR1CS_W_INV_LEFT operands); with it the device
 * evaluates the 2*fb*width + partial S-boxes of the permutation jointly - the state is carried as fractions over one
 * common denominator and all x, 1/x wires come out of ONE field inversion instead of one per S-box.  The wires
 * written are identical (tests/test_gpu_frontend.py::test_poseidon_joint_evaluation_equals_plain_program, tests/test_frontend.py). */
typedef struct {
    uint32_t width, full_rounds_beginning, partial_rounds, full_rounds_end;
    const uint8_t* mds;        /* width*width*32, row-major MDS_matrix[i][j] */
    const uint8_t* round_keys; /* (fb+partial+fe)*width*32 in consumption order */
} bpr1cs_poseidon_params;
typedef struct {
    uint32_t params;           /* index into poseidon_params */
    uint32_t in_lc[8];         /* ids (as in wops) of the `width` input linear combinations, before the first round key */
    const uint32_t* sbox_mul;  /* for every S-box in synthesis order: the multiplier whose (left, right) = (x, 1/x) */
} bpr1cs_poseidon_perm;

typedef struct {
    uint32_t n; /* multipliers (len a_L)          */
    uint32_t q; /* constraints                    */
    uint32_t m; /* committed variables V          */
    /* constraints, CSR by row: terms of constraint j are [row_off[j], row_off[j+1]) */
    const uint32_t* row_off;   /* q+1 */
    const uint32_t* term_var;  /* nnz : (kind<<28)|index */
    const uint8_t* term_coeff; /* nnz * 32 */
    /* optional witness program (NULL -> caller must pass wires to prove_batch) */
    const bpr1cs_wop* wops;   /* n */
    uint32_t n_lc;            /* number of linear combinations referenced by wops */
    const uint32_t* lc_off;   /* n_lc+1 */
    const uint32_t* lc_var;   /* terms */
    const uint8_t* lc_coeff;  /* terms * 32 */
    /* optional Poseidon annotations (zero / NULL when absent) */
    uint32_t n_poseidon_params;
    const bpr1cs_poseidon_params* poseidon_params;
    uint32_t n_poseidon_perms;
    const bpr1cs_poseidon_perm* poseidon_perms;
} bpr1cs_circuit_desc;

/* number of visible gfx950 devices (0 when none) */
int bpr1cs_device_count(void);
/* select the HIP device used by handles created afterwards on this thread */
int bpr1cs_set_device(int ordinal);

/* PedersenGens::default() + BulletproofGens::new(gens_capacity, 1)
 * (reference src/gadget_vsmt_4.rs:386-387); builds the fixed-base tables in HBM. */
int bpr1cs_gens_create(uint32_t gens_capacity, bpr1cs_gens** out);
void bpr1cs_gens_destroy(bpr1cs_gens* g);
uint32_t bpr1cs_gens_capacity(const bpr1cs_gens* g);
/* which: 0 = B, 1 = B_blinding, 2 = G[i], 3 = H[i]; compressed encoding */
int bpr1cs_gens_point(const bpr1cs_gens* g, int which, uint32_t i, uint8_t out[32]);

/* geometry of the handle's fixed-base tables: window bits W, windows per scalar, storage format (always 1: 27 limbs of 29 bits
 * in 128-byte slots), bytes */
int bpr1cs_gens_table_info(const bpr1cs_gens* g, uint32_t* window_bits, uint32_t* windows, uint32_t* format, uint64_t* bytes);
/* ---- options of a generator handle.  Every option has a default that is the measured optimum on MI355X (what bench.py runs);
 * value < 0 = back to that default.  No process-wide knobs exist: two threads on two handles never see each other's settings.
 * Results (proof bytes, verdicts) never depend on an option, with two exceptions: BPR1CS_OPT_VERIFY_GROUP_FALLBACK = 0 makes
 * bpr1cs_verify_batch return one verdict per GROUP of proofs (see there), and BPR1CS_OPT_CHECK_WITNESS = 1 replaces the bytes of a
 * proof nobody would accept by a record that says why. */
#define BPR1CS_OPT_UNFOLD_ROUNDS 0    /* IPA rounds computed from the UN-folded generator tables before the folded generators are
                                         materialised (default: 4 - measured 2 / 3 / 4 / 5 = 2420 / 2748 / 2880 / 2678 proofs/s -, every round for a job of
                                         at most 64 proofs with N x proofs <= 655 360, where a variable-base round is pure latency; clamped to lg N) */
#define BPR1CS_OPT_WITNESS_TEAM 2     /* lanes of a wavefront cooperating on one proof during witness synthesis: 4, 8 (default) or 16
                                         (measured 4 / 8 / 16 = 2941 / 2970 / 2939 proofs/s on one box) */
#define BPR1CS_OPT_TAIL_ROUNDS 3      /* how many of the LAST inner-product rounds (latency bound) a job enqueues on its own tail stream
                                         instead of the handle's heavy stream (default 7 = the rounds with m_k <= 64; 0 = none) */
#define BPR1CS_OPT_SHARED_BACK 4      /* 1 (default): the jobs in flight on a handle share the device scratch of their back phases, the wire /
                                         blinding vectors and the raw TranscriptRng output (each is live for a part of a job only) */
#define BPR1CS_OPT_FACTOR_VECTORS 5   /* measuring option: 0 (default) = closed form of the argument's factor vectors, the product scalars of
                                         an un-folded round produced by the MSM kernel where it fetches a term (from N = 4096 on; 3 =
                                         for every N); 2 = closed form, the scalars written out as N x B arrays by a kernel of their
                                         own (round 4); 1 = the factor vectors themselves as N x B arrays (what bpr1cs_ipa_create uses) */
#define BPR1CS_OPT_MSM_THREADS_LOG2 6 /* measuring option: log2 of the (chunk, proof) threads per launch of the MSM kernel (default 21) */
#define BPR1CS_OPT_JOB_PROOFS 7       /* proofs per device job when bpr1cs_prove_batch cuts a batch into jobs (default 0 = the largest of
                                         16384, 12288, 8192 ... 4096, 3584, 3072 ... 64 whose working set fits next to the tables:
                                         4096 for N = 32768 on 288 GB) */
#define BPR1CS_OPT_JOBS_IN_FLIGHT 8   /* device jobs bpr1cs_prove_batch keeps in flight: 1 or 2 (default 2: the latency-bound front of
                                         job k+1 runs next to the multiscalar multiplications of job k) */
#define BPR1CS_OPT_HOST_CHAIN_PROOFS 9 /* a job of up to this many proofs runs its TranscriptRng chains (2n + 8 strictly sequential Keccak-f[1600]
                                         per proof: 0.15-0.3 us each on an x86-64 core, 2.5 us on a GPU lane group) on host threads, one proof
                                         per thread, while the device takes the wires and computes A_I / A_O; the raw 64-byte draws are
                                         uploaded and reduced mod l on the device.  Default (-1): 4 proofs per CPU the process may use
                                         (affinity mask, cgroup quota); 0: never (the device chain, what a large batch hides behind the job
                                         before it).  The verifier likewise replays the transcripts of up to 8 proofs on the calling
                                         thread (public bytes only; 0 keeps them on the device).  Hashing, and for the verifier the
                                         reduction and inversion of its public challenges, only - no group arithmetic, and no arithmetic
                                         on a secret, ever runs on the host */
#define BPR1CS_OPT_HOST_CHAIN_SHARE 10 /* measuring option: percent (0..100) of a large job's proofs whose TranscriptRng chains run on host threads,
                                         eight proofs per AVX-512 register set, streamed to the device in chunks of draws while the rest run
                                         in k_rng_stream.  Default (-1), per job of bpr1cs_prove_batch: none without AVX-512 or with fewer than 2 worker threads
                                         (the process may use budget - 1 of its usable CPUs: affinity mask, cgroup quota).  The first job of
                                         a call has nothing to hide its chains behind: the host takes the part that lets its workers and the
                                         device end together (~39 % of 4096 depth-32 proofs on 15 workers), and none of a job that leaves the
                                         device at most one wavefront per SIMD (2 proofs each: 2048 on MI355X) or whose chains are too short
                                         to earn the hand-over back.  A job that follows another: the share the workers
                                         hash in 3/4 of the heavy stream's time per job measured so far in the call (its multiscalar
                                         launches; before any job has ended, the length of the device chain), at the rate the workers last
                                         measured - e.g. 100 % of a 4096-proof depth-32 job on 15 workers, ~55 % on 3.  A pinned share is
                                         honoured whenever there is a worker.  Jobs that BPR1CS_OPT_HOST_CHAIN_PROOFS puts on the host whole
                                         are not affected */
#define BPR1CS_OPT_WINDOW_BITS 16     /* creation only: signed window width W (4..15) of the fixed-base tables.  A term costs
                                         ceil(253/W) mixed additions; table bytes = (2+2*cap) * ceil(253/W) * (2^(W-1)+1) * 128
                                         (W=8: 35 GB, W=11: 198 GB at capacity 32768).  Default 0 = the widest W <= 15 whose tables fit in
                                         30 % of the free device memory, else the widest W <= 11 under 70 %: W = 15 for capacities up to
                                         1024 (9 / 37 / 73 GB and 0.4 / 1.2 / 2.5 s of table building at capacity 128 / 512 / 1024: the
                                         price of 17 instead of 23 additions per term for the small circuits' throughput), 11 for
                                         capacity 32768 on a 288 GB device, 8 / 7 for the reference's as-shipped tree depths (N = 131072 /
                                         262144, gadget_vsmt_4.rs:25, gadget_vsmt_2.rs:23).  A process that creates several handles, or
                                         wants small tables for a latency-only use, passes W explicitly (W = 8: 1/12 of the bytes) */
#define BPR1CS_OPT_SECRET_INDEPENDENT 11 /* creation only: 0 (default) or 1, anything else BPR1CS_ERR_INVALID_ARGUMENT.  1 = the commit phase of
                                         the prover - the V_j (in a prove job and in the pc_gens.commit shape of bpr1cs_msm_fixed: two terms
                                         over B and B~; its general form stays variable time), A_I1, A_O1, S1 with their blinding terms, and
                                         T_1, T_3, T_4, T_5, T_6 - runs through k_msm_fixed_ct: for a fixed (circuit, batch size, handle
                                         options) its sequence of memory addresses, branch outcomes and launched grids does not depend on
                                         committed values, wires, blindings or TranscriptRng draws (see TIMING SIDE CHANNELS above).  Same
                                         bytes as with 0.  Costs a second, narrow table set for all 2 + 2*cap bases (4-bit windows: 64 x 9
                                         slots x 128 B = 73.7 KB per base, 4.8 GB at capacity 32768), charged to the handle before W and the
                                         job size are chosen, and 64 instead of 23 additions per term over plain n-term sums */
#define BPR1CS_OPT_VERIFY_GROUP 12    /* proofs per group G of bpr1cs_verify_batch's grouped form.  Default 0; 0 and 1 = off (one mega-check
                                         per proof, 2N x windows table additions each); 2 .. 4096 (larger values are clamped) = the batch is
                                         cut into ceil(batch / G) groups of G consecutive proofs (the last may be short; G >= batch is one
                                         group), every group is checked by ONE combined identity test with per-proof weights - the
                                         shared-base sum is then 2N x windows additions per GROUP - and only the proofs of a group
                                         whose test fails are checked one by one.  Same verdicts as with 0 (an accepted group: every
                                         proof of it is valid but with probability <= 1/l over the weights, l the group order).  A
                                         call with batch = 1 takes the per-proof path.  Meant for groups of tens to a few hundred proofs
                                         (measured: 16 / 64 / 256): a group's own points are summed by ONE wavefront, so
                                         a group of thousands is a long serial chain - for one verdict over a whole large batch use
                                         bpr1cs_verify_batch_combined.  bpr1cs_verify_batch_combined, _scalars and
                                         _sharded ignore the option.
                                         SECURITY: the weights come from the derivation of bpr1cs_verify_batch_combined, seeded with
                                         the FIRST proof's 32 bytes of `verifier_rng_seeds` (index_base 0) and bound to every proof and
                                         commitment of the batch: with fresh per-proof seeds they are unpredictable to whoever made
                                         the proofs, as they are there; with `verifier_rng_seeds` = NULL (32 zero bytes) they are
                                         deterministic Fiat-Shamir values of the digest over every proof and commitment - the caveat
                                         that stands there for a constant batch seed */
#define BPR1CS_OPT_VERIFY_GROUP_FALLBACK 13 /* what the grouped form does with a group whose identity test fails or that holds a malformed
                                         proof.  1 (default): its proofs are re-checked by the per-proof path - the verdicts are those of
                                         BPR1CS_OPT_VERIFY_GROUP = 0.  0: no re-check, every proof of such a group gets verdict 0 (for a
                                         caller that rejects a whole submission unit anyway; the one setting under which verdicts depend
                                         on an option).  2: bisection on the device - same verdicts as 1, without the per-proof path.
                                         For a range R of proofs of one group let S(R) be the sum of rho_b x (proof b's mega-check
                                         point) over the well-formed proofs b of R.  A malformed proof (its format check or the
                                         decoding of one of its points fails) is part of no sum and gets verdict 0.  S(R) = identity:
                                         every well-formed proof of R gets 1.  A failing range of one proof: that proof gets 0.  A
                                         failing range of s > 1 proofs is split into its first ceil(s / 2) proofs and the rest:
                                         S(left) is computed - one column of the shared-base sum plus left's own points -,
                                         S(right) = S(R) - S(left) is a point subtraction, and both parts are treated the same way.
                                         The failing ranges of all groups at one depth share their launches (at most
                                         ceil(log2 G) <= 12 depths); a group with k bad proofs costs about k x ceil(log2 G) columns
                                         where 1 costs G, and a group whose only fault is a malformed proof costs nothing more.
                                         SECURITY: the sub-range tests reuse the group's weights rho_b, which were fixed after every
                                         proof of the batch was bound into the digest: a tested range that holds an invalid proof is
                                         accepted with probability <= 1/l, and the bound for a call is (number of ranges tested)/l.
                                         Values above 2 mean 1.  Without effect while BPR1CS_OPT_VERIFY_GROUP is off */
#define BPR1CS_VERIFY_GROUP_FALLBACK_NONE 0    /* values of BPR1CS_OPT_VERIFY_GROUP_FALLBACK */
#define BPR1CS_VERIFY_GROUP_FALLBACK_RECHECK 1
#define BPR1CS_VERIFY_GROUP_FALLBACK_BISECT 2
#define BPR1CS_OPT_CHECK_WITNESS 14   /* 0 (default; values < 0 too): off - the prove calls prove whatever they are given, as upstream's
                                         Prover::prove does: a witness that violates its circuit yields well-formed bytes no verifier
                                         accepts, and no signal.  1 (any other value means 1): every prove job checks its assignment on
                                         the device before its first commitment sum reads the wires - a_L[i] a_R[i] = a_O[i] for every
                                         multiplier i, and sum coeff x value = 0 for every constraint j (row j of the description's CSR;
                                         value(One) = 1, public inputs, committed values and wires taken as they were handed in or synthesised) - in
                                         bpr1cs_prove_batch, _transcripts, _draws and _begin / _end, for host wires and for the device
                                         witness program, on default and BPR1CS_OPT_SECRET_INDEPENDENT handles alike.  A proof whose
                                         assignment fails is REFUSED: its slot of `proofs_out` holds a refusal record instead of a
                                         proof (below) and bpr1cs_prove_stats.refused counts it.  Everything else is as with 0: the job
                                         runs the same launches, every other proof has the same bytes, commitments are written for
                                         every proof, a transcript handed in ends where it ends today, and the call returns what it
                                         returns today - one bad witness does not cost the other proofs of a call that is cut into
                                         jobs.  Costs two short kernels per job (one 32-byte read per constraint term and three per
                                         multiplier per proof; no multiplication for +-1 coefficients) and, once per circuit, the
                                         constraints by row on the device: 36 B per term, uploaded by the first checked job (measured:
                                         DESIGN.md 5.55).  Read once when a prove call starts, like every option */
/* Refusal record of BPR1CS_OPT_CHECK_WITNESS, bpr1cs_proof_len() bytes like a proof: byte 0 = BPR1CS_PROOF_REFUSED - a version byte
 * that bpr1cs_proof_parse and every verifier reject (BPR1CS_ERR_FORMAT / verdict 0) -, then little-endian 32-bit words at the
 * offsets below; every other byte is 0.  0xFFFFFFFF = no multiplier / no constraint is violated. */
#define BPR1CS_PROOF_REFUSED 0xFF
#define BPR1CS_REFUSAL_OFF_GATE 4          /* the lowest multiplier i with a_L[i] a_R[i] != a_O[i] */
#define BPR1CS_REFUSAL_OFF_ROW 8           /* the lowest constraint j with sum coeff x value != 0 */
#define BPR1CS_REFUSAL_OFF_GATE_COUNT 12   /* number of violated multipliers (saturating) */
#define BPR1CS_REFUSAL_OFF_ROW_COUNT 16    /* number of violated constraints (saturating) */
int bpr1cs_gens_set_option(bpr1cs_gens* g, int option, int value);
/* bpr1cs_gens_create with options: `pairs` = n_pairs x (option, value).  BPR1CS_ERR_INVALID_ARGUMENT for an unknown option. */
int bpr1cs_gens_create_opts(uint32_t gens_capacity, const int32_t* pairs, size_t n_pairs, bpr1cs_gens** out);
/* A handle keeps the device scratch of its prove jobs between calls (per job slot, shared front, shared back phase: ~19 MB per proof
 * of the depth-32 circuit, 80 GB at the default job size), so that no allocation happens in steady state.  This hands all of it to
 * the allocator's cache (bpr1cs_release_cached_memory then returns it to the driver); BPR1CS_ERR_INVALID_ARGUMENT while a job of
 * the handle is in flight.  The verifier entry points do it themselves when they find no memory. */
int bpr1cs_gens_release_scratch(bpr1cs_gens* g);
/* give the device memory cached by the library's allocator (freed tables, workspaces) back to the driver */
int bpr1cs_release_cached_memory(void);

/* Every index, offset and operand kind of `desc` is validated (constraint terms, witness program, linear combinations:
 * a multiplier's operands may only refer to committed values and to wires of EARLIER multipliers);
 * BPR1CS_ERR_INVALID_ARGUMENT otherwise.  poseidon_perm.sbox_mul must hold one entry per S-box of its parameter set. */
int bpr1cs_circuit_create(const bpr1cs_circuit_desc* desc, bpr1cs_circuit** out);
void bpr1cs_circuit_destroy(bpr1cs_circuit* c);
/* proof length in bytes: 1 + 32*(13 + 2*lg(next_pow2(n))) */
size_t bpr1cs_proof_len(const bpr1cs_circuit* c);

/* Batched Prover::commit x m  +  gadget synthesis  +  Prover::prove
 * (reference src/gadget_vsmt_4.rs:390-434), one independent transcript per proof.
 *   label              Transcript::new(label)
 *   values             batch * m * 32   committed values, proof-major (+ batch * p * 32 public inputs behind them, see "Public inputs";
 *                                       + batch * a * 32 auxiliary inputs behind those when wires == NULL, see "Auxiliary inputs")
 *   v_blindings        batch * m * 32
 *   rng_seeds          batch * 32       the 32 bytes upstream draws from thread_rng()
 *                                       in TranscriptRng::finalize (made explicit)
 *   wires              NULL (run the circuit's witness program on the device) or
 *                      batch * 3 * n * 32 : a_L | a_R | a_O per proof
 *   proofs_out         batch * bpr1cs_proof_len
 *   commitments_out    batch * m * 32 (may be NULL)
 * Any batch size: the call cuts the batch into device jobs of BPR1CS_OPT_JOB_PROOFS proofs (default: what fits next to the
 * tables) and keeps BPR1CS_OPT_JOBS_IN_FLIGHT of them in flight, so ONE call with a large batch runs the device at the rate
 * bench.py reports; if the device runs out of memory the jobs in flight are drained, the handle's scratch is handed back and
 * the job is tried again - then with half the job size for the rest of THIS call (the automatic choice is made afresh by the
 * next call).  Not while a job opened with bpr1cs_prove_batch_begin is in flight on the same handle
 * (BPR1CS_ERR_INVALID_ARGUMENT): the call needs both job slots of the handle and may release its arenas. */
int bpr1cs_prove_batch(const bpr1cs_gens* g, const bpr1cs_circuit* c, const uint8_t* label, size_t label_len,
                       const uint8_t* values, const uint8_t* v_blindings, const uint8_t* rng_seeds,
                       const uint8_t* wires, size_t batch, uint8_t* proofs_out, uint8_t* commitments_out);

/* The same with the caller's transcripts, for Prover::new(&pc_gens, &mut transcript) on a transcript that is not fresh
 * (reference src/gadget_vsmt_4.rs:390-391: `let mut prover_transcript = Transcript::new(b"VSMT"); Prover::new(&pc_gens,
 * &mut prover_transcript)` - any messages appended in between are part of the state).  `transcripts`: n_transcripts = batch
 * handles (proof i starts from transcripts[i] and leaves it in the state upstream's `&mut` transcript has when prove() returns;
 * a batch of one with its one transcript is this case), or n_transcripts = 1 < batch: every proof starts from a copy of
 * transcripts[0], which is left untouched. */
typedef struct bpr1cs_transcript bpr1cs_transcript;
int bpr1cs_prove_batch_transcripts(const bpr1cs_gens* g, const bpr1cs_circuit* c, bpr1cs_transcript* const* transcripts, size_t n_transcripts,
                                   const uint8_t* values, const uint8_t* v_blindings, const uint8_t* rng_seeds,
                                   const uint8_t* wires, size_t batch, uint8_t* proofs_out, uint8_t* commitments_out);

/* The same for a caller that runs the front of Prover::prove ITSELF, on the host, before the call: it has appended Prover::new's
 * ("dom-sep", "r1cs v1"), every commit's ("V", V_i) and prove's ("m", m as LE64) messages to transcripts[i] (bpr1cs_transcript_* below, or
 * its own merlin), and has drawn the proof's 2n + 8 `Scalar::random(&mut rng)` values from the TranscriptRng upstream builds there
 * (transcript.build_rng().rekey_with_witness_bytes("v_blinding", b_i) for every commitment, finalize(32 bytes of thread_rng())):
 * i_bl, o_bl, s_bl, s_L[0..n), s_R[0..n), the five t blindings - `draws` = batch x (2n + 8) x 64 raw bytes in that order, not reduced.
 * Why: that chain is 2n + 8 strictly sequential Keccak-f[1600] - 7 ms for a depth-32 tree proof, 57 ms at depth 253 on a host core - and
 * depends on nothing the gadget's synthesis produces: a caller that starts it on a thread of its own when its last commitment is made
 * (host/r1cs.hpp Prover does; a Rust shim would with merlin's own TranscriptRng) finds it finished when prove() is called.  The library
 * only reduces the draws mod l and proves; transcripts[i] is left where upstream's `&mut` transcript is after prove().  No commitments
 * are returned (the caller made them).  Same proof bytes as bpr1cs_prove_batch_transcripts with the same 32 bytes. */
int bpr1cs_prove_batch_draws(const bpr1cs_gens* g, const bpr1cs_circuit* c, bpr1cs_transcript* const* transcripts /* batch */,
                             const uint8_t* values, const uint8_t* v_blindings, const uint8_t* draws, const uint8_t* wires, size_t batch,
                             uint8_t* proofs_out);

/* Asynchronous form of bpr1cs_prove_batch: `begin` uploads the inputs and enqueues the whole prove on
 * one of two per-handle HIP stream pairs and returns without waiting; `end` waits for that job and
 * copies the results out.  Two jobs may be in flight per gens handle (a third `begin` before an `end` is refused with
 * BPR1CS_ERR_INVALID_ARGUMENT: a job owns one of the handle's two stream / buffer slots): the latency-bound phase of
 * batch k+1 (TranscriptRng Keccak chain, witness synthesis) then overlaps the VALU-bound MSM/IPA
 * phase of batch k.  Input buffers may be released as soon as `begin` returns.  (A job small enough for BPR1CS_OPT_HOST_CHAIN_PROOFS
 * hashes its TranscriptRng chains on host threads inside `begin`: the call then takes the chains' time - 7 ms for depth-32 proofs -
 * before it returns; set the option to 0 on a handle whose small jobs must be enqueued without that.) */
typedef struct bpr1cs_job bpr1cs_job;
int bpr1cs_prove_batch_begin(const bpr1cs_gens* g, const bpr1cs_circuit* c, const uint8_t* label, size_t label_len,
                             const uint8_t* values, const uint8_t* v_blindings, const uint8_t* rng_seeds,
                             const uint8_t* wires, size_t batch, bpr1cs_job** job_out);
int bpr1cs_prove_batch_end(bpr1cs_job* job, uint8_t* proofs_out, uint8_t* commitments_out);

/* Batched Verifier::verify (reference src/gadget_vsmt_4.rs:442-479): per proof, replay the transcript over the
 * commitments and the proof, flatten the constraints and evaluate the single mega-check multiscalar
 * multiplication; ok_out[i] = 1 iff proof i is accepted (R1CSError::VerificationError / FormatError -> 0).
 *   proofs               batch * bpr1cs_proof_len(c)
 *   commitments          batch * m * 32   the V's the verifier `commit`s, in gadget order (+ batch * p * 32 public inputs behind them)
 *   verifier_rng_seeds   batch * 32 or NULL (zeros): the 32 bytes upstream draws from thread_rng() for `r`
 * On a handle with BPR1CS_OPT_VERIFY_GROUP = G >= 2 a batch of 2 or more proofs is checked group by group - one combined identity
 * test per G consecutive proofs, the per-proof check only inside a group that fails: per-proof verdicts at close to the cost of
 * bpr1cs_verify_batch_combined while the proofs are good (see the option for the weights and BPR1CS_OPT_VERIFY_GROUP_FALLBACK).
 *
 * THE CALLER'S TRANSCRIPTS (Verifier::new(&mut transcript) on a transcript that is not fresh: it holds a session id, a nonce, the
 * proof before this one): bpr1cs_verify_batch, _combined, _scalars and _sharded take them in the two arguments they have.  With
 * BPR1CS_LABEL_TRANSCRIPTS set in `label_len`, `label` is a bpr1cs_transcript* const* (cast to const uint8_t*) of
 * count = label_len & ~BPR1CS_LABEL_TRANSCRIPTS handles, count = batch or 1:
 *   - proof b is replayed from the state of handle b (count = 1: every proof from handle 0) in place of Transcript::new(label);
 *     everything from ("dom-sep", "r1cs v1") on is what it is in the label form;
 *   - when the call returns BPR1CS_OK and count = batch (a batch of one with its one handle included), handle b is left in the state
 *     after proof b's last inner-product challenge: where upstream's `&mut` transcript is when verify() returns (its build_rng works
 *     on a clone) and where bpr1cs_prove_batch_transcripts leaves the prover's handle - so the next proof of a protocol is proved
 *     and verified on the same pair of transcripts.  The handle of a REJECTED or malformed proof is advanced in the same way (the replay
 *     absorbs every element whatever it finds; upstream leaves the transcript wherever the error struck): only the handle of an
 *     accepted proof is meaningful to continue from;
 *   - count = 1 < batch leaves the handle untouched, and a call that returns an error touches no handle;
 *   - BPR1CS_ERR_INVALID_ARGUMENT: a count other than 1 or batch, a NULL handle, the same handle twice when count = batch (which
 *     state would it be left in?), and the flag on bpr1cs_prove_batch / bpr1cs_prove_batch_begin (bpr1cs_prove_batch_transcripts is
 *     their form of it).
 * The grouped form seeds its weights as in the label form.  A transcript's contents are public for a verifier: nothing is wiped.
 * Without the flag every call is what it was (a label_len of 2^63 or more has never been a label). */
#define BPR1CS_LABEL_TRANSCRIPTS ((size_t)1 << (sizeof(size_t) * 8 - 1))
int bpr1cs_verify_batch(const bpr1cs_gens* g, const bpr1cs_circuit* c, const uint8_t* label, size_t label_len,
                        const uint8_t* proofs, const uint8_t* commitments, const uint8_t* verifier_rng_seeds, size_t batch,
                        int* ok_out);

/* Cross-proof batched verification (SURVEY §8a P10 "batchable across proofs", §8e; the reference verifies one proof
 * at a time, gadget_vsmt_4.rs:479).  With per-proof weights rho_j the `batch` mega-checks collapse into one: the 2N+2
 * shared bases B, B~, G_i, H_i get ONE combined scalar each (sum_j rho_j * scalar_j) and a single fixed-base MSM; only
 * the proofs' own points are handled per proof.  The weights, in Merlin transcripts (<- appends, u64 = 8 bytes LE):
 *   bind_j  = the proof's own verifier transcript after its last inner-product challenge, cloned,
 *             <- ("ipp_a", a) <- ("ipp_b", b); challenge_bytes("bpr1cs-bind", 32)   (every byte of proof and commitments - and, the
 *             clone being of the proof's OWN transcript, the state it started from: a label or the caller's transcript alike)
 *   leaf_g  = Transcript("bpr1cs batch leaf") <- u64("leaf", g) <- ("proof", bind_j) for the 32 proofs j = 32g .. 32g+31
 *             (the last leaf may be short); challenge_bytes("leaf", 32).  A circuit with p > 0 public inputs: after each
 *             proof's ("proof", bind_j) the leaf absorbs ("public", p_j,0 || ... || p_j,p-1) (p x 32 bytes) - the proof's own
 *             transcript does not hold them, and the B scalar is linear in them: with unbound public inputs and a constant
 *             batch seed, whoever picks them after seeing the weights could cancel two invalid proofs against each other.
 *             p = 0: no such message, the derivation is what it was
 *   D       = Transcript("bpr1cs batch verify") <- ("seed", batch_seed) <- u64("base", index_base) <- u64("count", batch)
 *             <- ("leaf", leaf_g) for every leaf in order; challenge_bytes("digest", 32)
 *   rho_j   = Transcript("bpr1cs batch weight") <- ("digest", D) <- u64("j", index_base + j); challenge_scalar("rho")
 * (csrc/kernels.hpp K_verify_transcript, K_batch_leaf, K_batch_digest, K_batch_weights; tests/verify_scalar_cases.py holds the
 * same derivation over the oracle's Merlin and checks the combined scalars against it byte for byte.)
 * SECURITY: `batch_seed` must be 32 bytes of FRESH SECRET randomness drawn by the verifier after the proofs were
 * received (e.g. getrandom); the weights are derived from it together with a binding value of every proof and
 * commitment of the batch, so they cannot be predicted by whoever produced the proofs.  A public or constant seed
 * only leaves the binding (deterministic, proof-dependent weights).  `verifier_rng_seeds` = NULL likewise makes
 * each proof's own challenge r deterministic; pass fresh randomness in production.
 * Output: this caller's partial point (32-byte compressed) and whether all proofs were well-formed.  A job sharded
 * over several GPUs gives every rank a disjoint `index_base` range, gathers the ranks' points (RCCL all_gather of
 * 32 bytes per rank, see bulletproofs-r1cs-gadgets_amd/sharding.py) and accepts iff bpr1cs_points_sum of them is the
 * identity (32 zero bytes) and every rank was well-formed.  A failing batch is then re-checked with
 * bpr1cs_verify_batch to find the culprit (BPR1CS_OPT_VERIFY_GROUP does both in one call on one device). */
int bpr1cs_verify_batch_combined(const bpr1cs_gens* gens, const bpr1cs_circuit* circuit, const uint8_t* label, size_t label_len,
                                 const uint8_t* proofs, const uint8_t* commitments, const uint8_t* verifier_rng_seeds,
                                 const uint8_t* batch_seed /* 32 */, uint64_t index_base, size_t batch,
                                 uint8_t* partial_point_out /* 32 */, int* wellformed_out);
/* Multi-GPU form: the same checks, but instead of evaluating the shared-base part itself the caller gets
 *   combined_scalars_out  (2N+2)*32 canonical scalars in base order B, B_blinding, G[0..N), H[0..N)   (N = padded n)
 *   own_points_sum_out    the weighted sum of its proofs' own points (A_I1.., V, T, L, R), compressed
 * The ranks add their scalar vectors (all_reduce / all_gather + bpr1cs_scalars_sum, ~2 MB at N = 32768), every rank
 * evaluates a 1/world slice of the bases with bpr1cs_msm_fixed(bases [first, first+count), batch 1), the slice points
 * and the own-points sums are gathered, and the job is accepted iff bpr1cs_points_sum of all of them is the identity
 * and every rank was well-formed.  The shared-base MSM is then computed ONCE per job instead of once per rank. */
int bpr1cs_verify_batch_scalars(const bpr1cs_gens* gens, const bpr1cs_circuit* circuit, const uint8_t* label, size_t label_len,
                                const uint8_t* proofs, const uint8_t* commitments, const uint8_t* verifier_rng_seeds,
                                const uint8_t* batch_seed /* 32 */, uint64_t index_base, size_t batch,
                                uint8_t* combined_scalars_out, uint8_t* own_points_sum_out /* 32 */, int* wellformed_out);
/* out[i] = sum_r vectors[r*len + i] mod l   (count vectors of len canonical scalars; host side) */
int bpr1cs_scalars_sum(const uint8_t* vectors, size_t count, size_t len, uint8_t* out);

/* ---- the path's only exchange step behind the C ABI (north star: "RCCL over xGMI only for the batched-verifier
 * final MSM").  One process per GPU; a bpr1cs_comm is an RCCL communicator: either created here from the 128-byte unique id
 * that rank 0 draws and hands to the others out of band (exactly ncclGetUniqueId / ncclCommInitRank), or an ncclComm_t the
 * host already has (passed as void*; the header needs no rccl.h, the library loads librccl on first use).
 * bpr1cs_verify_batch_sharded = the whole multi-GPU batched verifier in one call per rank, every rank with its own proofs:
 * bpr1cs_verify_batch_scalars -> ncclAllGather of the scalar vectors ((2N+2)*32 bytes per rank) -> sum mod l -> this rank's
 * 1/world slice of the shared bases (bpr1cs_msm_fixed) -> ncclAllGather of 65 bytes per rank -> *accepted_out = 1 iff the sum
 * of all points is the identity and every rank was well-formed (the same verdict on every rank).  `index_base`: disjoint
 * per rank (e.g. rank * batch).  comm = NULL: a job of one rank (no RCCL involved).  Collective: every rank of the
 * communicator must call it; a rank whose local part fails still takes part in both all_gathers and makes the job fail.
 * The reference verifies one proof at a time on one core (src/gadget_vsmt_4.rs:479). */
typedef struct bpr1cs_comm bpr1cs_comm;
int bpr1cs_comm_unique_id(uint8_t id_out[128]);
int bpr1cs_comm_create(const uint8_t id[128], int rank, int world, bpr1cs_comm** out);
int bpr1cs_comm_wrap(void* nccl_comm, int rank, int world, bpr1cs_comm** out); /* not destroyed by bpr1cs_comm_destroy */
void bpr1cs_comm_destroy(bpr1cs_comm* comm);
int bpr1cs_verify_batch_sharded(const bpr1cs_gens* gens, const bpr1cs_circuit* circuit, const uint8_t* label, size_t label_len,
                                const uint8_t* proofs, const uint8_t* commitments, const uint8_t* verifier_rng_seeds,
                                const uint8_t* batch_seed /* 32 */, uint64_t index_base, size_t batch, const bpr1cs_comm* comm,
                                int* accepted_out);

/* `count` native Poseidon permutations (reference Poseidon_permutation, gadget_poseidon.rs:189-280; sbox_inverse
 * selects SboxType::Inverse / Cube): inputs/outputs are count*width canonical scalars.  With the Inverse S-box each
 * permutation costs ONE inversion (state carried as fractions, as in the witness program).  Used by the sparse
 * Merkle tree builders of bpr1cs_gadgets.h to hash a whole tree level per call. */
int bpr1cs_poseidon_permutation_batch(const bpr1cs_poseidon_params* params, int sbox_inverse, const uint8_t* inputs, size_t count,
                                      uint8_t* outputs);
/* ---- low-level entry points for parity tests and for a Rust shim -------------------------------------------
 * merlin::Transcript (merlin 2.0: STROBE-128 over Keccak-f[1600]) exactly as the prover kernels run it; host-side. */
bpr1cs_transcript* bpr1cs_transcript_new(const uint8_t* label, size_t label_len);                 /* Transcript::new(label)      */
void bpr1cs_transcript_free(bpr1cs_transcript* t);
void bpr1cs_transcript_append_message(bpr1cs_transcript* t, const uint8_t* label, size_t label_len, const uint8_t* msg, size_t msg_len);
void bpr1cs_transcript_challenge_bytes(bpr1cs_transcript* t, const uint8_t* label, size_t label_len, uint8_t* out, size_t out_len);
bpr1cs_transcript* bpr1cs_transcript_clone(const bpr1cs_transcript* t);                                 /* Transcript: Clone          */
/* merlin::TranscriptRng: t.build_rng().rekey_with_witness_bytes(witness_label, w_j) for j < count (witnesses: count x witness_len bytes)
 * .finalize(seed); fill_bytes = `count` successive RngCore::fill_bytes(len) calls (a draw of 64 bytes is one Scalar::random) */
typedef struct bpr1cs_transcript_rng bpr1cs_transcript_rng;
bpr1cs_transcript_rng* bpr1cs_transcript_build_rng(const bpr1cs_transcript* t, const uint8_t* witness_label, size_t label_len,
                                                   const uint8_t* witnesses, size_t witness_len, size_t count, const uint8_t seed[32]);
void bpr1cs_transcript_rng_fill_bytes(bpr1cs_transcript_rng* r, uint8_t* out, size_t len, size_t count);
void bpr1cs_transcript_rng_free(bpr1cs_transcript_rng* r);
/* InnerProductProof::create(transcript, &Q, G_factors, H_factors, G, H, a, b) of the bulletproofs crate (the last step of
 * every Prover::prove, reference src/gadget_vsmt_4.rs:434) for ONE proof over the handle's generators G[0..n), H[0..n):
 * appends ("dom-sep","ipp v1"), ("n", n) to `t`, runs the lg n rounds on the device (appending L_k, R_k and drawing u_k),
 * leaves `t` in the state the caller's protocol continues from.  n: a power of two <= capacity; scalars canonical.
 * L_out / R_out: lg n compressed points each; a_out / b_out: the final scalars. */
int bpr1cs_ipa_create(const bpr1cs_gens* g, bpr1cs_transcript* t, const uint8_t* Q /* 32, compressed */, const uint8_t* G_factors /* n*32 */,
                      const uint8_t* H_factors /* n*32 */, const uint8_t* a /* n*32 */, const uint8_t* b /* n*32 */, size_t n,
                      uint8_t* L_out /* lg n * 32 */, uint8_t* R_out /* lg n * 32 */, uint8_t* a_out /* 32 */, uint8_t* b_out /* 32 */);
/* RistrettoPoint::vartime_multiscalar_mul over arbitrary (compressed) points: out = sum_i scalars[i] * points[i], on the
 * device: Straus with shared doublings (as the variable-base IPA rounds) below 4096 terms, from there on Pippenger with the
 * 512 signed-digit buckets of a window staged in LDS (26 windows x chunks workgroups; lanes that meet in a bucket take turns).
 * BPR1CS_ERR_FORMAT if a point does not decode. */
int bpr1cs_msm(const uint8_t* scalars /* n*32 canonical */, const uint8_t* points /* n*32 compressed */, size_t n, uint8_t* out /* 32 */);

/* out = compress(sum of `count` compressed ristretto points); BPR1CS_ERR_FORMAT if one of them does not decode */
int bpr1cs_points_sum(const uint8_t* points, size_t count, uint8_t* out);

/* Low-level, for parity tests and a Rust shim: out = sum_t scalars[t] * Base(bases[t])
 * for `batch` independent scalar vectors over the SAME fixed bases; base index:
 * 0 = B, 1 = B_blinding, 2+i = G[i], 2+capacity+i = H[i].
 * (replaces RistrettoPoint::multiscalar_mul over the generators). */
int bpr1cs_msm_fixed(const bpr1cs_gens* g, const uint32_t* bases, size_t terms, const uint8_t* scalars /* batch*terms*32 */,
                     size_t batch, uint8_t* out /* batch*32 */);

/* ---- proof wire format: R1CSProof::to_bytes / from_bytes of the bulletproofs crate behind the reference's
 * typed helpers (src/gadget_bound_check.rs:49-116, src/gadget_set_membership.rs:93-171).  Version byte 0 = one-phase (the
 * phase-2 commitments are the identity and are not written; what this library's prover emits), 1 = two-phase.  Points are
 * kept as their 32-byte encodings (not decoded, as upstream); scalars must be canonical. */
typedef struct {
    uint8_t A_I1[32], A_O1[32], S1[32];
    uint8_t A_I2[32], A_O2[32], S2[32]; /* all zero (identity) in a one-phase proof */
    uint8_t T_1[32], T_3[32], T_4[32], T_5[32], T_6[32];
    uint8_t t_x[32], t_x_blinding[32], e_blinding[32];
    uint32_t lg_n;                      /* rounds of the inner-product proof, < 32 */
    uint8_t L[32][32], R[32][32];
    uint8_t ipp_a[32], ipp_b[32];
} bpr1cs_proof;
/* BPR1CS_ERR_FORMAT: unknown version byte, (len-1) not a multiple of 32, too few / an odd number of IPA elements,
 * lg_n >= 32, or a non-canonical scalar. */
int bpr1cs_proof_parse(const uint8_t* bytes, size_t len, bpr1cs_proof* out);
size_t bpr1cs_proof_serialized_len(const bpr1cs_proof* p);
/* one-phase form when A_I2 = A_O2 = S2 = identity, two-phase form otherwise (as R1CSProof::to_bytes) */
int bpr1cs_proof_serialize(const bpr1cs_proof* p, uint8_t* out, size_t cap, size_t* len_out);

/* diagnostic: number of Poseidon permutations of this circuit's witness program that are evaluated jointly
 * (test knob, environment: BPR1CS_WITNESS_MACRO=0 makes bpr1cs_circuit_create ignore the annotations) */
int bpr1cs_circuit_macro_perms(const bpr1cs_circuit* c);

/* Statistics of the last bpr1cs_prove_batch / bpr1cs_prove_batch_end that returned on the calling thread (HIP events), summed over the
 * device jobs of the call, for bench.py's roofline object. */
typedef struct {
    uint32_t jobs;          /* device jobs the call was cut into */
    uint32_t job_proofs;    /* proofs of the largest job */
    float phase_ms[6];      /* [0]=total [1]=inputs+V commitments [2]=RNG stream || witness synthesis [3]=commit MSMs [4]=polys [5]=IPA */
    double msm_ms;          /* summed launch durations of the dominant kernel (k_msm_fixed2), events recorded on its own stream */
    uint64_t msm_launches;
    uint64_t msm_terms;     /* scalar*point terms it processed, summed over the batch */
    uint64_t msm_adds;      /* table additions = terms x windows of the table a term reads (a circuit's merged tables may be narrower) */
    uint64_t host_chains;   /* proofs whose TranscriptRng chain ran on a host thread (BPR1CS_OPT_HOST_CHAIN_PROOFS) */
    /* why the jobs have the size they have (BPR1CS_OPT_JOB_PROOFS = 0: chosen from the free memory; all 0 when the size was given):
     * the largest candidate J with J * sizing_bytes_per_proof + sizing_fixed_bytes <= sizing_free_bytes was taken.  A caller that gets
     * smaller jobs than bench.py (4096 for N = 32768 on 288 GB) reads here what else was holding device memory when the handle sized them */
    uint64_t sizing_free_bytes;      /* device memory free (+ what the handle and the allocator's cache already hold) when the size was chosen */
    uint64_t sizing_bytes_per_proof; /* working set per proof: own fronts of the jobs in flight + shared front + back phase */
    uint64_t sizing_fixed_bytes;     /* per-job constants, the circuit's merged tables if still to be built, the 4 GiB that must stay free */
    uint64_t refused;       /* proofs the call refused because their assignment violates the circuit (BPR1CS_OPT_CHECK_WITNESS; 0 while it is off) */
} bpr1cs_prove_stats;
int bpr1cs_last_prove_stats(bpr1cs_prove_stats* out);

/* diagnostic: sustained rates of the device (each probe runs for about `seconds_each`, long enough for the clock to settle
 * to its power budget): lane-operations per second of v_mad_i64_i32 with every SIMD busy, and table additions (ge_madd_t
 * chains on register operands) per second - the integer ceilings bench.py prices the fixed-base MSM kernel against. */
int bpr1cs_device_rates(double seconds_each, double* mad_lane_ops_per_s, double* table_adds_per_s);

#ifdef __cplusplus
}
#endif
#endif
