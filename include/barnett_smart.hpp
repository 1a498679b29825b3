// barnett_smart.hpp -- header-only C++ mirror of the reference's trait surface for the hot path, over the C ABI of
// libmpshuffle.so.  Same names, argument meaning and error behaviour as
//   trait BarnettSmartProtocol { fn setup; fn shuffle_and_remask; fn verify_shuffle; }
//   [REF barnett-smart-card-protocol/src/lib.rs:74-78, 181-197] as implemented by DLCards<C>
//   [REF barnett-smart-card-protocol/src/discrete_log_cards/mod.rs:105-121, 380-443].
// Result<T, E> becomes: return T, throw E.
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "mpshuffle.h"

namespace barnett_smart {

// proof_essentials::error::CryptoError::ProofVerificationError(String)   [REF src/discrete_log_cards/tests.rs:223-225]
struct CryptoError : std::runtime_error {
  std::string check;
  explicit CryptoError(const std::string& name) : std::runtime_error("ProofVerificationError(" + name + ")"), check(name) {}
};
// CardProtocolError::{ProofVerificationError(CryptoError), IoError(String)}   [REF src/error.rs:6-12]
struct CardProtocolError : std::runtime_error {
  explicit CardProtocolError(const std::string& io) : std::runtime_error("IoError: " + io) {}
};

typedef std::array<uint8_t, 32> Scalar;        // C::ScalarField, little-endian canonical
typedef std::vector<uint8_t> ZKProofShuffle;   // shuffle::proof::Proof

struct Permutation {                            // utils::permutation::Permutation
  std::vector<uint32_t> mapping;                // permute_array(v)[i] = v[mapping[i]]
};

struct Parameters {                             // discrete_log_cards::Parameters [REF mod.rs:37-61]
  uint32_t m = 0, n = 0;
  std::vector<uint8_t> raw;                     // G | ck_0..ck_{n-1} | H | gen
};

// PB = wire bytes of an affine point on the curve: 64 for the 256-bit curves, 96 for BLS12-377 (mp_point_size)
template <size_t PB>
class DLCardsT {
 public:
  typedef std::array<uint8_t, PB> PublicKey;        // el_gamal::PublicKey (affine point)
  typedef std::array<uint8_t, 2 * PB> MaskedCard;   // el_gamal::Ciphertext(pub Affine, pub Affine)

  explicit DLCardsT(int curve_id = MP_CURVE_STARK, int device = 0) : curve_(curve_id) {
    if (mp_point_size(curve_id) != PB) throw CardProtocolError("curve / point size mismatch");
    if (mp_ctx_create(curve_id, device, &ctx_) != MP_OK) throw CardProtocolError(mp_last_error());
  }
  // The same over a device pool (mpshuffle.h "device pool"): devices[i] is the device of member i, a device named several times gives
  // lanes on it.  shuffle_and_remask_batch / verify_shuffle_batch cut their proofs into blocks over the members -- same bytes, same
  // status words --, every other member runs on member 0.
  DLCardsT(int curve_id, const std::vector<int>& devices) : curve_(curve_id) {
    if (mp_point_size(curve_id) != PB) throw CardProtocolError("curve / point size mismatch");
    if (mp_pool_create(curve_id, devices.size(), devices.data(), &pool_) != MP_OK) throw CardProtocolError(mp_last_error());
    ctx_ = mp_pool_member_ctx(pool_, 0);
  }
  ~DLCardsT() {
    unbind();
    if (pool_) mp_pool_destroy(pool_);      // (its contexts go with it)
    else mp_ctx_destroy(ctx_);
  }
  DLCardsT(const DLCardsT&) = delete;
  DLCardsT& operator=(const DLCardsT&) = delete;

  // fn setup<R: Rng>(rng, m, n) -> Result<Parameters, CardProtocolError>
  Parameters setup(const std::array<uint8_t, 32>& rng_seed, uint32_t m, uint32_t n) {
    Parameters pp;
    pp.m = m;
    pp.n = n;
    pp.raw.resize(mp_params_size_curve(curve_, n));
    if (mp_setup(ctx_, m, n, rng_seed.data(), pp.raw.data()) != MP_OK) throw CardProtocolError(mp_last_error());
    return pp;
  }

  // fn shuffle_and_remask<R: Rng>(rng, pp, shared_key, deck, masking_factors, permutation)
  //     -> Result<(Vec<MaskedCard>, ZKProofShuffle), CardProtocolError>
  std::pair<std::vector<MaskedCard>, ZKProofShuffle> shuffle_and_remask(const std::array<uint8_t, 32>& rng_seed, const Parameters& pp,
                                                                        const PublicKey& shared_key, const std::vector<MaskedCard>& deck,
                                                                        const std::vector<Scalar>& masking_factors,
                                                                        const Permutation& permutation) {
    const size_t N = (size_t)pp.m * pp.n;
    if (deck.size() != N || masking_factors.size() != N || permutation.mapping.size() != N)
      throw CardProtocolError("deck, masking factors and permutation must have m*n entries");
    bind(pp, shared_key);
    std::vector<MaskedCard> out(N);
    ZKProofShuffle proof(mp_proof_size_curve(curve_, pp.m, pp.n));
    int rc = mp_shuffle_and_remask(table_, deck[0].data(), masking_factors[0].data(), permutation.mapping.data(), rng_seed.data(),
                                   out[0].data(), proof.data());
    if (rc != MP_OK) throw CardProtocolError(mp_last_error());
    return {std::move(out), std::move(proof)};
  }

  // fn verify_shuffle(pp, shared_key, original_deck, shuffled_deck, proof) -> Result<(), CryptoError>
  void verify_shuffle(const Parameters& pp, const PublicKey& shared_key, const std::vector<MaskedCard>& original_deck,
                      const std::vector<MaskedCard>& shuffled_deck, const ZKProofShuffle& proof) {
    const size_t N = (size_t)pp.m * pp.n;
    if (original_deck.size() != N || shuffled_deck.size() != N) throw CardProtocolError("decks must have m*n entries");
    bind(pp, shared_key);
    int rc = mp_verify_shuffle(table_, original_deck[0].data(), shuffled_deck[0].data(), proof.data(), proof.size());
    if (rc > 0) throw CryptoError(mp_check_name(rc));
    if (rc < 0) throw CardProtocolError(mp_last_error());
  }

  // CanonicalSerialize / CanonicalDeserialize of ZKProofShuffle and `proof.serialized_size()`
  // [REF src/lib.rs:71; examples/parameter_selection.rs:95]
  size_t serialized_size(const Parameters& pp) const { return mp_serialized_proof_size(curve_, pp.m, pp.n); }
  std::vector<uint8_t> serialize(const Parameters& pp, const ZKProofShuffle& proof) const {
    std::vector<uint8_t> out(serialized_size(pp));
    if (proof.size() != mp_proof_size_curve(curve_, pp.m, pp.n) || mp_proof_serialize(curve_, pp.m, pp.n, proof.data(), out.data()) != MP_OK)
      throw CardProtocolError(mp_last_error());
    return out;
  }
  ZKProofShuffle deserialize_proof(const Parameters& pp, const std::vector<uint8_t>& bytes) const {
    ZKProofShuffle proof(mp_proof_size_curve(curve_, pp.m, pp.n));
    if (mp_proof_deserialize(curve_, pp.m, pp.n, bytes.data(), bytes.size(), proof.data()) != MP_OK) throw CardProtocolError(mp_last_error());
    return proof;
  }
  // The same for batches held as canonical bytes, converted ON THE DEVICE (mpshuffle.h "canonical serialisation"): `data` = B proofs of
  // serialized_size(pp) bytes / D decks of mp_serialized_deck_size bytes, back to back.  Status words are returned, not thrown: 0, or
  // MP_ERR_BAD_ENCODING for an entry that is refused (its refused elements are zero bytes in `wire`)
  struct Deserialized {
    std::vector<uint8_t> wire;
    std::vector<int32_t> status;
  };
  Deserialized deserialize_proofs(const Parameters& pp, const std::vector<uint8_t>& data) {
    const size_t B = serialized_size(pp) ? data.size() / serialized_size(pp) : 0;
    if (!B || B * serialized_size(pp) != data.size()) throw CardProtocolError("whole serialised proofs expected");
    Deserialized r{std::vector<uint8_t>(B * mp_proof_size_curve(curve_, pp.m, pp.n)), std::vector<int32_t>(B)};
    if (mp_proofs_deserialize_batch(ctx_, pp.m, pp.n, B, data.data(), r.wire.data(), r.status.data()) != MP_OK)
      throw CardProtocolError(mp_last_error());
    return r;
  }
  Deserialized deserialize_decks(const Parameters& pp, const std::vector<uint8_t>& data) {
    const size_t cards = (size_t)pp.m * pp.n, sz = mp_serialized_deck_size(curve_, cards), D = data.size() / sz;
    if (!D || D * sz != data.size()) throw CardProtocolError("whole serialised decks expected");
    Deserialized r{std::vector<uint8_t>(D * cards * 2 * PB), std::vector<int32_t>(D)};
    if (mp_decks_deserialize_batch(ctx_, D, cards, data.data(), r.wire.data(), r.status.data()) != MP_OK)
      throw CardProtocolError(mp_last_error());
    return r;
  }
  // device pointers: pass-throughs on this instance's context (mp_points_serialize_dev, mp_deck_serialize_dev, mp_proof_serialize_dev,
  // mp_proof_deserialize_dev); enqueued, final after sync()
  void points_serialize_dev(size_t count, const void* d_wire_points, void* d_out, void* d_status) {
    if (mp_points_serialize_dev(ctx_, count, d_wire_points, d_out, d_status) != MP_OK) throw CardProtocolError(mp_last_error());
  }
  void deck_serialize_dev(size_t decks, size_t cards, const void* d_wire_decks, void* d_out, void* d_status) {
    if (mp_deck_serialize_dev(ctx_, decks, cards, d_wire_decks, d_out, d_status) != MP_OK) throw CardProtocolError(mp_last_error());
  }
  void proof_serialize_dev(const Parameters& pp, size_t B, const void* d_proofs_wire, void* d_out, void* d_status) {
    if (mp_proof_serialize_dev(ctx_, pp.m, pp.n, B, d_proofs_wire, d_out, d_status) != MP_OK) throw CardProtocolError(mp_last_error());
  }
  void proof_deserialize_dev(const Parameters& pp, size_t B, const void* d_data, void* d_out_proofs_wire, void* d_status) {
    if (mp_proof_deserialize_dev(ctx_, pp.m, pp.n, B, d_data, d_out_proofs_wire, d_status) != MP_OK) throw CardProtocolError(mp_last_error());
  }
  void sync() {
    if (mp_sync(ctx_) != MP_OK) throw CardProtocolError(mp_last_error());
  }

  // Opening cards in batches (mpshuffle.h "opening cards"): compute_reveal_token / unmask [REF mod.rs:300-378] for the T tokens of
  // many cards in one call each.  signer[c T + j] = index into keys of the player whose token j of card c is; tokens, proofs and
  // status words come in that order.  Pass-throughs on the table of (pp, shared_key): status words are returned, not thrown.
  typedef PublicKey RevealToken;
  typedef std::array<uint8_t, 2 * PB + 32> ZKProofReveal;
  struct RevealedTokens {
    std::vector<RevealToken> tokens;
    std::vector<ZKProofReveal> proofs;
    std::vector<int32_t> status;
  };
  struct OpenedCards {
    std::vector<PublicKey> plaintexts;          // c1 - sum of the card's tokens; zero bytes for a card that was not opened
    std::vector<uint32_t> index;                // place in card_list, 0xFFFFFFFF = not there
    std::vector<int32_t> token_status, card_status;
  };
  RevealedTokens compute_reveal_tokens(const std::vector<std::array<uint8_t, 32>>& rng_seeds, const Parameters& pp, const PublicKey& shared_key,
                                       const std::vector<PublicKey>& keys, const std::vector<std::array<uint8_t, 32>>& secret_keys,
                                       const std::vector<MaskedCard>& cards, const std::vector<uint32_t>& signer) {
    if (cards.empty() || signer.empty() || signer.size() % cards.size() || keys.empty() || secret_keys.size() != keys.size() ||
        rng_seeds.size() != signer.size())
      throw CardProtocolError("compute_reveal_tokens: the same number of signers for every card, one seed per token, one secret per key");
    bind(pp, shared_key);
    RevealedTokens r{std::vector<RevealToken>(signer.size()), std::vector<ZKProofReveal>(signer.size()), std::vector<int32_t>(signer.size())};
    if (mp_reveal_batch(table_, keys.size(), keys[0].data(), secret_keys[0].data(), cards.size(), cards[0].data(),
                        (uint32_t)(signer.size() / cards.size()), signer.data(), rng_seeds[0].data(), r.tokens[0].data(), r.proofs[0].data(),
                        r.status.data()) != MP_OK)
      throw CardProtocolError(mp_last_error());
    return r;
  }
  OpenedCards open_cards(const Parameters& pp, const PublicKey& shared_key, const std::vector<PublicKey>& keys, const std::vector<MaskedCard>& cards,
                         const std::vector<uint32_t>& signer, const std::vector<RevealToken>& tokens, const std::vector<ZKProofReveal>& proofs,
                         const std::vector<PublicKey>& card_list) {
    if (cards.empty() || signer.empty() || signer.size() % cards.size() || keys.empty() || tokens.size() != signer.size() ||
        proofs.size() != signer.size())
      throw CardProtocolError("open_cards: the same number of signers for every card, one token and one proof per signer");
    bind(pp, shared_key);
    OpenedCards o{std::vector<PublicKey>(cards.size()), std::vector<uint32_t>(cards.size()), std::vector<int32_t>(signer.size()),
                  std::vector<int32_t>(cards.size())};
    if (mp_unmask_batch(table_, keys.size(), keys[0].data(), cards.size(), cards[0].data(), (uint32_t)(signer.size() / cards.size()),
                        signer.data(), tokens[0].data(), proofs[0].data(), card_list.size(), card_list.empty() ? nullptr : card_list[0].data(),
                        o.plaintexts[0].data(), o.index.data(), o.token_status.data(), o.card_status.data()) != MP_OK)
      throw CardProtocolError(mp_last_error());
    return o;
  }
  // The same for cards with different numbers of tokens (mp_reveal_ragged_batch, mp_unmask_ragged_batch): counts[c] tokens for card c,
  // signers, seeds, tokens, proofs and status words in lane order -- those of card c follow those of card c - 1.
  RevealedTokens compute_reveal_tokens(const std::vector<std::array<uint8_t, 32>>& rng_seeds, const Parameters& pp, const PublicKey& shared_key,
                                       const std::vector<PublicKey>& keys, const std::vector<std::array<uint8_t, 32>>& secret_keys,
                                       const std::vector<MaskedCard>& cards, const std::vector<uint32_t>& signer,
                                       const std::vector<uint32_t>& counts) {
    const std::vector<uint32_t> first = ragged_first(counts, cards.size(), signer.size(), "compute_reveal_tokens");
    if (keys.empty() || secret_keys.size() != keys.size() || rng_seeds.size() != signer.size())
      throw CardProtocolError("compute_reveal_tokens: one seed per token, one secret per key");
    bind(pp, shared_key);
    RevealedTokens r{std::vector<RevealToken>(signer.size()), std::vector<ZKProofReveal>(signer.size()), std::vector<int32_t>(signer.size())};
    if (mp_reveal_ragged_batch(table_, keys.size(), keys[0].data(), secret_keys[0].data(), cards.size(), cards[0].data(), first.data(),
                               signer.data(), rng_seeds[0].data(), r.tokens[0].data(), r.proofs[0].data(), r.status.data()) != MP_OK)
      throw CardProtocolError(mp_last_error());
    return r;
  }
  OpenedCards open_cards(const Parameters& pp, const PublicKey& shared_key, const std::vector<PublicKey>& keys, const std::vector<MaskedCard>& cards,
                         const std::vector<uint32_t>& signer, const std::vector<RevealToken>& tokens, const std::vector<ZKProofReveal>& proofs,
                         const std::vector<PublicKey>& card_list, const std::vector<uint32_t>& counts) {
    const std::vector<uint32_t> first = ragged_first(counts, cards.size(), signer.size(), "open_cards");
    if (keys.empty() || tokens.size() != signer.size() || proofs.size() != signer.size())
      throw CardProtocolError("open_cards: one token and one proof per signer");
    bind(pp, shared_key);
    OpenedCards o{std::vector<PublicKey>(cards.size()), std::vector<uint32_t>(cards.size()), std::vector<int32_t>(signer.size()),
                  std::vector<int32_t>(cards.size())};
    if (mp_unmask_ragged_batch(table_, keys.size(), keys[0].data(), cards.size(), cards[0].data(), first.data(), signer.data(), tokens[0].data(),
                               proofs[0].data(), card_list.size(), card_list.empty() ? nullptr : card_list[0].data(), o.plaintexts[0].data(),
                               o.index.data(), o.token_status.data(), o.card_status.data()) != MP_OK)
      throw CardProtocolError(mp_last_error());
    return o;
  }

  // Dealing and seating in batches (mpshuffle.h "dealing and seating"): mask / verify_mask / remask / verify_remask [REF mod.rs:182-298]
  // for the cards of many tables, and compute_aggregate_key [REF mod.rs:167-180] for many tables, in one call each.  Card i goes under
  // shared_keys[key_index[i]].  Pass-throughs on a table of pp (of the parameters only G is used): status words are returned, not thrown.
  typedef std::array<uint8_t, 2 * PB + 32> ZKProofMasking;      // (ZKProofRemasking is the same type: a Chaum-Pedersen proof)
  typedef std::array<uint8_t, PB + 32> ZKProofKeyOwnership;
  struct DealtCards {
    std::vector<MaskedCard> cards;              // zero bytes for a lane whose status is not 0
    std::vector<ZKProofMasking> proofs;
    std::vector<int32_t> status;
  };
  struct AggregateKeys {
    std::vector<PublicKey> keys;                // zero bytes for a table whose status is not 0
    std::vector<int32_t> player_status, table_status;
  };
  DealtCards deal(const std::vector<std::array<uint8_t, 32>>& rng_seeds, const Parameters& pp, const std::vector<PublicKey>& shared_keys,
                  const std::vector<uint32_t>& key_index, const std::vector<PublicKey>& cards, const std::vector<Scalar>& factors) {
    return mask_batch(MP_DEAL_MASK, rng_seeds, pp, shared_keys, key_index, cards.size(), cards.empty() ? nullptr : cards[0].data(), factors);
  }
  std::vector<int32_t> verify_deal(const Parameters& pp, const std::vector<PublicKey>& shared_keys, const std::vector<uint32_t>& key_index,
                                   const std::vector<PublicKey>& cards, const std::vector<MaskedCard>& masked_cards,
                                   const std::vector<ZKProofMasking>& proofs) {
    return verify_mask_batch(MP_DEAL_MASK, pp, shared_keys, key_index, cards.size(), cards.empty() ? nullptr : cards[0].data(), masked_cards, proofs);
  }
  DealtCards deal_remask(const std::vector<std::array<uint8_t, 32>>& rng_seeds, const Parameters& pp, const std::vector<PublicKey>& shared_keys,
                         const std::vector<uint32_t>& key_index, const std::vector<MaskedCard>& masked_cards, const std::vector<Scalar>& factors) {
    return mask_batch(MP_DEAL_REMASK, rng_seeds, pp, shared_keys, key_index, masked_cards.size(),
                      masked_cards.empty() ? nullptr : masked_cards[0].data(), factors);
  }
  std::vector<int32_t> verify_deal_remask(const Parameters& pp, const std::vector<PublicKey>& shared_keys, const std::vector<uint32_t>& key_index,
                                          const std::vector<MaskedCard>& original_cards, const std::vector<MaskedCard>& remasked_cards,
                                          const std::vector<ZKProofMasking>& proofs) {
    return verify_mask_batch(MP_DEAL_REMASK, pp, shared_keys, key_index, original_cards.size(),
                             original_cards.empty() ? nullptr : original_cards[0].data(), remasked_cards, proofs);
  }
  // The same four by index: the keys are the slots of a key set of the table bound now (key_set below), key_index[i] names a slot
  // (mp_mask_batch_keyset, mp_verify_mask_batch_keyset); a card on an empty slot reads MP_ERR_BAD_ARGUMENT
  DealtCards deal(const std::vector<std::array<uint8_t, 32>>& rng_seeds, const mp_keyset* ks, const std::vector<uint32_t>& key_index,
                  const std::vector<PublicKey>& cards, const std::vector<Scalar>& factors) {
    return mask_batch_keyset(MP_DEAL_MASK, rng_seeds, ks, key_index, cards.size(), cards.empty() ? nullptr : cards[0].data(), factors);
  }
  std::vector<int32_t> verify_deal(const mp_keyset* ks, const std::vector<uint32_t>& key_index, const std::vector<PublicKey>& cards,
                                   const std::vector<MaskedCard>& masked_cards, const std::vector<ZKProofMasking>& proofs) {
    return verify_mask_batch_keyset(MP_DEAL_MASK, ks, key_index, cards.size(), cards.empty() ? nullptr : cards[0].data(), masked_cards, proofs);
  }
  DealtCards deal_remask(const std::vector<std::array<uint8_t, 32>>& rng_seeds, const mp_keyset* ks, const std::vector<uint32_t>& key_index,
                         const std::vector<MaskedCard>& masked_cards, const std::vector<Scalar>& factors) {
    return mask_batch_keyset(MP_DEAL_REMASK, rng_seeds, ks, key_index, masked_cards.size(), masked_cards.empty() ? nullptr : masked_cards[0].data(),
                             factors);
  }
  std::vector<int32_t> verify_deal_remask(const mp_keyset* ks, const std::vector<uint32_t>& key_index, const std::vector<MaskedCard>& original_cards,
                                          const std::vector<MaskedCard>& remasked_cards, const std::vector<ZKProofMasking>& proofs) {
    return verify_mask_batch_keyset(MP_DEAL_REMASK, ks, key_index, original_cards.size(),
                                    original_cards.empty() ? nullptr : original_cards[0].data(), remasked_cards, proofs);
  }
  // seating straight into a key set (mp_keyset_seat_ragged_batch): the sum of table k goes into slot slots[k] on the device;
  // slot_status[k] is 0, the table's word, or MP_ERR_BAD_ENCODING for a sum that is the identity -- the slot is empty then
  struct SeatedKeys {
    AggregateKeys sums;
    std::vector<int32_t> slot_status;
  };
  SeatedKeys seat(mp_keyset* ks, const std::vector<uint32_t>& slots, const std::vector<uint32_t>& players, const std::vector<PublicKey>& keys,
                  const std::vector<ZKProofKeyOwnership>& proofs, const std::vector<std::array<uint8_t, 32>>& fs_init) {
    const std::vector<uint32_t> first = ragged_first(players, players.size(), keys.size(), "seat");
    if (proofs.size() != keys.size() || fs_init.size() != keys.size() || slots.size() != players.size())
      throw CardProtocolError("seat: one proof and one digest per player, one slot per table");
    const size_t tables = players.size();
    SeatedKeys s{AggregateKeys{std::vector<PublicKey>(tables), std::vector<int32_t>(keys.size()), std::vector<int32_t>(tables)},
                 std::vector<int32_t>(tables)};
    if (mp_keyset_seat_ragged_batch(ks, tables, first.data(), slots.data(), keys[0].data(), proofs[0].data(), fs_init[0].data(), s.sums.keys[0].data(),
                                    s.sums.player_status.data(), s.sums.table_status.data(), s.slot_status.data()) != MP_OK)
      throw CardProtocolError(mp_last_error());
    return s;
  }
  // tables x players, lane = table * players + seat; fs_init[lane] = Blake2s("Key Ownership Proof" || player_public_info) (mp_blake2s)
  AggregateKeys compute_aggregate_keys(const Parameters& pp, size_t players, const std::vector<PublicKey>& keys,
                                       const std::vector<ZKProofKeyOwnership>& proofs, const std::vector<std::array<uint8_t, 32>>& fs_init) {
    if (!players || keys.empty() || keys.size() % players || proofs.size() != keys.size() || fs_init.size() != keys.size())
      throw CardProtocolError("compute_aggregate_keys: the same number of players at every table, one proof and one digest per player");
    bind_any(pp, keys[0]);
    const size_t tables = keys.size() / players;
    AggregateKeys a{std::vector<PublicKey>(tables), std::vector<int32_t>(keys.size()), std::vector<int32_t>(tables)};
    if (mp_aggregate_keys_batch(table_, tables, (uint32_t)players, keys[0].data(), proofs[0].data(), fs_init[0].data(), a.keys[0].data(),
                                a.player_status.data(), a.table_status.data()) != MP_OK)
      throw CardProtocolError(mp_last_error());
    return a;
  }
  // tables of different sizes (mp_aggregate_keys_ragged_batch): players[k] players at table k, the lanes of table k after those of k - 1
  AggregateKeys compute_aggregate_keys(const Parameters& pp, const std::vector<uint32_t>& players, const std::vector<PublicKey>& keys,
                                       const std::vector<ZKProofKeyOwnership>& proofs, const std::vector<std::array<uint8_t, 32>>& fs_init) {
    const std::vector<uint32_t> first = ragged_first(players, players.size(), keys.size(), "compute_aggregate_keys");
    if (proofs.size() != keys.size() || fs_init.size() != keys.size())
      throw CardProtocolError("compute_aggregate_keys: one proof and one digest per player");
    bind_any(pp, keys[0]);
    const size_t tables = players.size();
    AggregateKeys a{std::vector<PublicKey>(tables), std::vector<int32_t>(keys.size()), std::vector<int32_t>(tables)};
    if (mp_aggregate_keys_ragged_batch(table_, tables, first.data(), keys[0].data(), proofs[0].data(), fs_init[0].data(), a.keys[0].data(),
                                       a.player_status.data(), a.table_status.data()) != MP_OK)
      throw CardProtocolError(mp_last_error());
    return a;
  }

  // Secrets drawn on the device from seeds (mpshuffle.h "secrets drawn on the device from seeds", the stream is defined there): one
  // fresh 32-byte CSPRNG seed per shuffle / per player, never reused, and all a caller has to store.  Pass-throughs: status words are
  // returned, not thrown.
  struct ShuffleWitnesses {
    std::vector<Permutation> permutations;          // one per seed, m*n entries each
    std::vector<std::vector<Scalar>> masking_factors;
  };
  struct SeededShuffles {
    std::vector<std::vector<MaskedCard>> decks;
    std::vector<ZKProofShuffle> proofs;
    std::vector<int32_t> status;
  };
  struct PlayerKeys {
    std::vector<PublicKey> keys;
    std::vector<Scalar> secret_keys;
    std::vector<ZKProofKeyOwnership> proofs;        // empty without fs_init
    std::vector<int32_t> status;
  };
  // [REF examples/round.rs:265-266] for many shuffles: what shuffle_and_remask_batch_seeded uses for the same seeds
  ShuffleWitnesses sample_shuffle_witnesses(const std::vector<std::array<uint8_t, 32>>& seeds, const Parameters& pp) {
    const size_t N = (size_t)pp.m * pp.n, B = seeds.size();
    if (!B) throw CardProtocolError("sample_shuffle_witnesses: at least one seed");
    bind_any(pp, generator(pp));
    std::vector<Scalar> sc(B * N);
    std::vector<uint32_t> pm(B * N);
    if (mp_sample_secrets_batch(table_, B, seeds[0].data(), (uint32_t)N, (uint32_t)N, sc[0].data(), pm.data()) != MP_OK)
      throw CardProtocolError(mp_last_error());
    ShuffleWitnesses w{std::vector<Permutation>(B), std::vector<std::vector<Scalar>>(B)};
    for (size_t b = 0; b < B; ++b) {
      w.permutations[b].mapping.assign(pm.begin() + b * N, pm.begin() + (b + 1) * N);
      w.masking_factors[b].assign(sc.begin() + b * N, sc.begin() + (b + 1) * N);
    }
    return w;
  }
  // shuffle_and_remask for many decks under one aggregate key, the witness of proof b drawn from seeds[b], which is also its prover seed
  SeededShuffles shuffle_and_remask_batch_seeded(const std::vector<std::array<uint8_t, 32>>& seeds, const Parameters& pp, const PublicKey& shared_key,
                                                 const std::vector<std::vector<MaskedCard>>& decks) {
    const size_t N = (size_t)pp.m * pp.n, B = seeds.size();
    if (!B || decks.size() != B) throw CardProtocolError("shuffle_and_remask_batch_seeded: one deck per seed, at least one");
    std::vector<MaskedCard> in(B * N), out(B * N);
    for (size_t b = 0; b < B; ++b) {
      if (decks[b].size() != N) throw CardProtocolError("shuffle_and_remask_batch_seeded: a deck has m*n cards");
      std::copy(decks[b].begin(), decks[b].end(), in.begin() + b * N);
    }
    bind(pp, shared_key);
    const size_t psz = mp_proof_size_curve(curve_, pp.m, pp.n);
    std::vector<uint8_t> proofs(B * psz);
    SeededShuffles r{std::vector<std::vector<MaskedCard>>(B), std::vector<ZKProofShuffle>(B), std::vector<int32_t>(B)};
    if (mp_shuffle_and_remask_batch_seeded(table_, B, nullptr, in[0].data(), seeds[0].data(), out[0].data(), proofs.data(), r.status.data(),
                                           nullptr, nullptr) != MP_OK)
      throw CardProtocolError(mp_last_error());
    for (size_t b = 0; b < B; ++b) {
      r.decks[b].assign(out.begin() + b * N, out.begin() + (b + 1) * N);
      r.proofs[b].assign(proofs.begin() + b * psz, proofs.begin() + (b + 1) * psz);
    }
    return r;
  }
  // player_keygen [REF mod.rs:123-130] for many players; with fs_init (one Blake2s("Key Ownership Proof" || player_public_info) per seed)
  // also prove_key_ownership [REF mod.rs:132-149] under the prover seed seeds[k]
  PlayerKeys player_keygen_batch(const std::vector<std::array<uint8_t, 32>>& seeds, const Parameters& pp,
                                 const std::vector<std::array<uint8_t, 32>>& fs_init = {}) {
    const size_t K = seeds.size();
    if (!K || (!fs_init.empty() && fs_init.size() != K)) throw CardProtocolError("player_keygen_batch: at least one seed; one digest per seed, or none");
    bind_any(pp, generator(pp));
    PlayerKeys p{std::vector<PublicKey>(K), std::vector<Scalar>(K), std::vector<ZKProofKeyOwnership>(fs_init.size()), std::vector<int32_t>(K)};
    if (mp_keygen_batch(table_, K, seeds[0].data(), fs_init.empty() ? nullptr : fs_init[0].data(), p.keys[0].data(), p.secret_keys[0].data(),
                        fs_init.empty() ? nullptr : p.proofs[0].data(), p.status.data()) != MP_OK)
      throw CardProtocolError(mp_last_error());
    return p;
  }

  // shuffle_and_remask / verify_shuffle for many decks under one aggregate key (mp_*_batch; through the pool when there is one).
  // Status words are returned, not thrown: 0, the code of the first failing check (mp_check_name), or < 0.
  struct Shuffles {
    std::vector<std::vector<MaskedCard>> decks;
    std::vector<ZKProofShuffle> proofs;
    std::vector<int32_t> status;
  };
  Shuffles shuffle_and_remask_batch(const std::vector<std::array<uint8_t, 32>>& rng_seeds, const Parameters& pp, const PublicKey& shared_key,
                                    const std::vector<std::vector<MaskedCard>>& decks, const std::vector<std::vector<Scalar>>& masking_factors,
                                    const std::vector<Permutation>& permutations) {
    const size_t N = (size_t)pp.m * pp.n, B = rng_seeds.size();
    if (!B || decks.size() != B || masking_factors.size() != B || permutations.size() != B)
      throw CardProtocolError("shuffle_and_remask_batch: one deck, one factor list and one permutation per seed, at least one");
    std::vector<MaskedCard> in(B * N), out(B * N);
    std::vector<Scalar> rho(B * N);
    std::vector<uint32_t> perm(B * N);
    for (size_t b = 0; b < B; ++b) {
      if (decks[b].size() != N || masking_factors[b].size() != N || permutations[b].mapping.size() != N)
        throw CardProtocolError("deck, masking factors and permutation must have m*n entries");
      std::copy(decks[b].begin(), decks[b].end(), in.begin() + b * N);
      std::copy(masking_factors[b].begin(), masking_factors[b].end(), rho.begin() + b * N);
      std::copy(permutations[b].mapping.begin(), permutations[b].mapping.end(), perm.begin() + b * N);
    }
    bind(pp, shared_key);
    const size_t psz = mp_proof_size_curve(curve_, pp.m, pp.n);
    std::vector<uint8_t> proofs(B * psz);
    Shuffles r{std::vector<std::vector<MaskedCard>>(B), std::vector<ZKProofShuffle>(B), std::vector<int32_t>(B)};
    const int rc = ptable_ ? mp_pool_shuffle_and_remask_batch(ptable_, B, nullptr, in[0].data(), rho[0].data(), perm.data(), rng_seeds[0].data(),
                                                              out[0].data(), proofs.data(), r.status.data())
                           : mp_shuffle_and_remask_batch(table_, B, in[0].data(), rho[0].data(), perm.data(), rng_seeds[0].data(), out[0].data(),
                                                         proofs.data(), r.status.data());
    if (rc != MP_OK) throw CardProtocolError(mp_last_error());
    for (size_t b = 0; b < B; ++b) {
      r.decks[b].assign(out.begin() + b * N, out.begin() + (b + 1) * N);
      r.proofs[b].assign(proofs.begin() + b * psz, proofs.begin() + (b + 1) * psz);
    }
    return r;
  }
  std::vector<int32_t> verify_shuffle_batch(const Parameters& pp, const PublicKey& shared_key, const std::vector<std::vector<MaskedCard>>& original_decks,
                                            const std::vector<std::vector<MaskedCard>>& shuffled_decks, const std::vector<ZKProofShuffle>& proofs) {
    const size_t N = (size_t)pp.m * pp.n, B = proofs.size(), psz = mp_proof_size_curve(curve_, pp.m, pp.n);
    if (!B || original_decks.size() != B || shuffled_decks.size() != B)
      throw CardProtocolError("verify_shuffle_batch: one deck and one shuffled deck per proof, at least one");
    std::vector<MaskedCard> in(B * N), shuf(B * N);
    std::vector<uint8_t> pf(B * psz);
    for (size_t b = 0; b < B; ++b) {
      if (original_decks[b].size() != N || shuffled_decks[b].size() != N || proofs[b].size() != psz)
        throw CardProtocolError("decks must have m*n entries and proofs their wire length");
      std::copy(original_decks[b].begin(), original_decks[b].end(), in.begin() + b * N);
      std::copy(shuffled_decks[b].begin(), shuffled_decks[b].end(), shuf.begin() + b * N);
      std::copy(proofs[b].begin(), proofs[b].end(), pf.begin() + b * psz);
    }
    bind(pp, shared_key);
    std::vector<int32_t> status(B);
    const int rc = ptable_ ? mp_pool_verify_shuffle_batch(ptable_, B, nullptr, in[0].data(), shuf[0].data(), pf.data(), status.data())
                           : mp_verify_shuffle_batch(table_, B, in[0].data(), shuf[0].data(), pf.data(), status.data());
    if (rc != MP_OK) throw CardProtocolError(mp_last_error());
    return status;
  }

  // The shuffle chains of many tables, of different lengths, in one call (mp_verify_shuffle_chain_ragged): table t brings links + 1 decks
  // (deck j + 1 the output of link j), one proof per link and its aggregate key.  -> per table the status words of its links, those of
  // verify_shuffle_batch link by link.
  struct Chain {
    PublicKey shared_key;
    std::vector<std::vector<MaskedCard>> decks;
    std::vector<ZKProofShuffle> proofs;
  };
  std::vector<std::vector<int32_t>> verify_shuffle_chains(const Parameters& pp, const std::vector<Chain>& chains) {
    const size_t N = (size_t)pp.m * pp.n, psz = mp_proof_size_curve(curve_, pp.m, pp.n);
    if (chains.empty()) throw CardProtocolError("verify_shuffle_chains: at least one table");
    std::vector<uint32_t> links;
    std::vector<MaskedCard> decks;
    std::vector<PublicKey> keys;
    std::vector<uint8_t> pf;
    for (const Chain& ch : chains) {
      if (ch.proofs.empty() || ch.decks.size() != ch.proofs.size() + 1)
        throw CardProtocolError("verify_shuffle_chains: a chain is at least one link: links + 1 decks and one proof per link");
      links.push_back((uint32_t)ch.proofs.size());
      for (const std::vector<MaskedCard>& d : ch.decks) {
        if (d.size() != N) throw CardProtocolError("decks must have m*n entries and proofs their wire length");
        decks.insert(decks.end(), d.begin(), d.end());
      }
      for (const ZKProofShuffle& p : ch.proofs) {
        if (p.size() != psz) throw CardProtocolError("decks must have m*n entries and proofs their wire length");
        pf.insert(pf.end(), p.begin(), p.end());
        keys.push_back(ch.shared_key);
      }
    }
    bind_any(pp, chains[0].shared_key);
    std::vector<int32_t> status(keys.size());
    if (mp_verify_shuffle_chain_ragged(table_, chains.size(), links.data(), keys[0].data(), decks[0].data(), pf.data(), status.data()) != MP_OK)
      throw CardProtocolError(mp_last_error());
    std::vector<std::vector<int32_t>> out;
    size_t o = 0;
    for (uint32_t n : links) {
      out.emplace_back(status.begin() + o, status.begin() + o + n);
      o += n;
    }
    return out;
  }
  // The same over device arrays in the table-major layout of mp_verify_shuffle_chain_ragged_dev (16-byte aligned; d_keys: one key per
  // link; any_key: a key of pp, to bind the table); links is a host vector.  Enqueued: d_status is final after sync().
  void verify_shuffle_chains_dev(const Parameters& pp, const PublicKey& any_key, const std::vector<uint32_t>& links, const void* d_keys,
                                 const void* d_decks, const void* d_proofs, void* d_status) {
    if (links.empty()) throw CardProtocolError("verify_shuffle_chains_dev: at least one table");
    bind_any(pp, any_key);
    if (mp_verify_shuffle_chain_ragged_dev(table_, links.size(), links.data(), d_keys, d_decks, d_proofs, d_status) != MP_OK)
      throw CardProtocolError(mp_last_error());
  }
  // how verify_shuffle_chains[_dev] cut their chains on the table bound now: MP_CHAIN_PIECES_WHOLE or MP_CHAIN_PIECES_BINARY (cut only where that saves passes); same words
  void set_chain_pieces(int mode) {
    if (!table_ || mp_set_chain_pieces(table_, mode) != MP_OK) throw CardProtocolError(table_ ? mp_last_error() : "set_chain_pieces: no table bound yet");
  }

  // Key sets whose slots change (mpshuffle.h): a set of `capacity` empty slots on the table of `pp` (any_key: a key of pp, to bind the
  // table).  It belongs to that table: key_set_close it before another Parameters value is bound.  key_set_update -> one status word
  // per key: MP_OK, or MP_ERR_BAD_ENCODING for a refused key, whose slot is EMPTY afterwards; a malformed slots vector throws.
  mp_keyset* key_set(const Parameters& pp, const PublicKey& any_key, size_t capacity) {
    bind_any(pp, any_key);
    mp_keyset* ks = nullptr;
    if (mp_keyset_create_empty(table_, capacity, &ks) != MP_OK) throw CardProtocolError(mp_last_error());
    return ks;
  }
  std::vector<int32_t> key_set_update(mp_keyset* ks, const std::vector<uint32_t>& slots, const std::vector<PublicKey>& keys) {
    if (slots.empty() || keys.size() != slots.size()) throw CardProtocolError("key_set_update: at least one slot, one key per slot");
    std::vector<int32_t> status(slots.size());
    if (mp_keyset_update(ks, slots.size(), slots.data(), keys[0].data(), status.data()) != MP_OK) throw CardProtocolError(mp_last_error());
    return status;
  }
  void key_set_update_dev(mp_keyset* ks, const std::vector<uint32_t>& slots, const void* d_keys, void* d_status) {
    if (mp_keyset_update_dev(ks, slots.size(), slots.data(), d_keys, d_status) != MP_OK) throw CardProtocolError(mp_last_error());
  }
  void key_set_clear(mp_keyset* ks, const std::vector<uint32_t>& slots) {
    if (mp_keyset_clear(ks, slots.size(), slots.data()) != MP_OK) throw CardProtocolError(mp_last_error());
  }
  size_t key_set_live(const mp_keyset* ks) const { return mp_keyset_live(ks); }
  void key_set_close(mp_keyset* ks) { mp_keyset_destroy(ks); }
  // verify_shuffle_chains with the key of table t named as slot key_index[t] of a key set of the table bound now (Chain::shared_key is
  // not read); every link of a table on an empty slot or past the set reads MP_ERR_BAD_ARGUMENT
  std::vector<std::vector<int32_t>> verify_shuffle_chains(const Parameters& pp, const mp_keyset* ks, const std::vector<uint32_t>& key_index,
                                                          const std::vector<Chain>& chains) {
    const size_t N = (size_t)pp.m * pp.n, psz = mp_proof_size_curve(curve_, pp.m, pp.n);
    if (chains.empty() || key_index.size() != chains.size()) throw CardProtocolError("verify_shuffle_chains: at least one table, one index per table");
    std::vector<uint32_t> links;
    std::vector<MaskedCard> decks;
    std::vector<uint8_t> pf;
    for (const Chain& ch : chains) {
      if (ch.proofs.empty() || ch.decks.size() != ch.proofs.size() + 1)
        throw CardProtocolError("verify_shuffle_chains: a chain is at least one link: links + 1 decks and one proof per link");
      links.push_back((uint32_t)ch.proofs.size());
      for (const std::vector<MaskedCard>& d : ch.decks) {
        if (d.size() != N) throw CardProtocolError("decks must have m*n entries and proofs their wire length");
        decks.insert(decks.end(), d.begin(), d.end());
      }
      for (const ZKProofShuffle& p : ch.proofs) {
        if (p.size() != psz) throw CardProtocolError("decks must have m*n entries and proofs their wire length");
        pf.insert(pf.end(), p.begin(), p.end());
      }
    }
    std::vector<int32_t> status(pf.size() / psz);
    if (!table_ || mp_verify_shuffle_chain_ragged_keyset(table_, ks, chains.size(), links.data(), key_index.data(), decks[0].data(), pf.data(),
                                                         status.data()) != MP_OK)
      throw CardProtocolError(table_ ? mp_last_error() : "verify_shuffle_chains: the key set's table is not bound");
    std::vector<std::vector<int32_t>> out;
    size_t o = 0;
    for (uint32_t n : links) {
      out.emplace_back(status.begin() + o, status.begin() + o + n);
      o += n;
    }
    return out;
  }

  mp_table* table() const { return table_; }   // for the batched / device-resident entry points of mpshuffle.h
  mp_pool_table* pool_table() const { return ptable_; }      // NULL without a device list

 private:
  DealtCards mask_batch(int kind, const std::vector<std::array<uint8_t, 32>>& rng_seeds, const Parameters& pp, const std::vector<PublicKey>& shared_keys,
                        const std::vector<uint32_t>& key_index, size_t count, const uint8_t* inputs, const std::vector<Scalar>& factors) {
    if (!count || shared_keys.empty() || key_index.size() != count || factors.size() != count || rng_seeds.size() != count)
      throw CardProtocolError("deal: at least one key and one card; one key index, one factor and one seed per card");
    bind_any(pp, shared_keys[0]);
    DealtCards d{std::vector<MaskedCard>(count), std::vector<ZKProofMasking>(count), std::vector<int32_t>(count)};
    if (mp_mask_batch(table_, kind, shared_keys.size(), shared_keys[0].data(), count, key_index.data(), inputs, factors[0].data(),
                      rng_seeds[0].data(), d.cards[0].data(), d.proofs[0].data(), d.status.data()) != MP_OK)
      throw CardProtocolError(mp_last_error());
    return d;
  }
  std::vector<int32_t> verify_mask_batch(int kind, const Parameters& pp, const std::vector<PublicKey>& shared_keys,
                                         const std::vector<uint32_t>& key_index, size_t count, const uint8_t* inputs,
                                         const std::vector<MaskedCard>& masked_cards, const std::vector<ZKProofMasking>& proofs) {
    if (!count || shared_keys.empty() || key_index.size() != count || masked_cards.size() != count || proofs.size() != count)
      throw CardProtocolError("verify_deal: at least one key and one card; one key index, one masked card and one proof per card");
    bind_any(pp, shared_keys[0]);
    std::vector<int32_t> status(count);
    if (mp_verify_mask_batch(table_, kind, shared_keys.size(), shared_keys[0].data(), count, key_index.data(), inputs, masked_cards[0].data(),
                             proofs[0].data(), status.data()) != MP_OK)
      throw CardProtocolError(mp_last_error());
    return status;
  }
  DealtCards mask_batch_keyset(int kind, const std::vector<std::array<uint8_t, 32>>& rng_seeds, const mp_keyset* ks, const std::vector<uint32_t>& key_index,
                               size_t count, const uint8_t* inputs, const std::vector<Scalar>& factors) {
    if (!count || !table_ || key_index.size() != count || factors.size() != count || rng_seeds.size() != count)
      throw CardProtocolError("deal: the key set's table bound, at least one card; one slot, one factor and one seed per card");
    DealtCards d{std::vector<MaskedCard>(count), std::vector<ZKProofMasking>(count), std::vector<int32_t>(count)};
    if (mp_mask_batch_keyset(table_, ks, kind, count, key_index.data(), inputs, factors[0].data(), rng_seeds[0].data(), d.cards[0].data(),
                             d.proofs[0].data(), d.status.data()) != MP_OK)
      throw CardProtocolError(mp_last_error());
    return d;
  }
  std::vector<int32_t> verify_mask_batch_keyset(int kind, const mp_keyset* ks, const std::vector<uint32_t>& key_index, size_t count,
                                                const uint8_t* inputs, const std::vector<MaskedCard>& masked_cards,
                                                const std::vector<ZKProofMasking>& proofs) {
    if (!count || !table_ || key_index.size() != count || masked_cards.size() != count || proofs.size() != count)
      throw CardProtocolError("verify_deal: the key set's table bound, at least one card; one slot, one masked card and one proof per card");
    std::vector<int32_t> status(count);
    if (mp_verify_mask_batch_keyset(table_, ks, kind, count, key_index.data(), inputs, masked_cards[0].data(), proofs[0].data(), status.data()) != MP_OK)
      throw CardProtocolError(mp_last_error());
    return status;
  }
  // the offsets array of the ragged calls: item c owns the lanes first[c] .. first[c+1] - 1
  static std::vector<uint32_t> ragged_first(const std::vector<uint32_t>& counts, size_t items, size_t lanes, const char* who) {
    std::vector<uint32_t> first(counts.size() + 1, 0);
    uint64_t sum = 0;
    bool ok = !counts.empty() && counts.size() == items;
    for (size_t i = 0; i < counts.size(); ++i) {
      ok = ok && counts[i] >= 1;
      sum += counts[i];
      first[i + 1] = (uint32_t)sum;
    }
    if (!ok || sum != lanes) throw CardProtocolError(std::string(who) + ": counts must name at least one lane for every item, and all of them");
    return first;
  }
  // G of the parameters: the key of a table that is bound for calls that use no key
  static PublicKey generator(const Parameters& pp) {
    PublicKey g{};
    if (pp.raw.size() >= PB) std::copy(pp.raw.begin(), pp.raw.begin() + PB, g.begin());
    return g;
  }
  // a table of pp, whatever its key: the calls that use only G of the parameters keep the one that is bound
  void bind_any(const Parameters& pp, const PublicKey& pk) {
    if (table_ && pp.raw == bound_params_ && pp.m == bound_m_) return;
    bind(pp, pk);
  }
  void bind(const Parameters& pp, const PublicKey& pk) {
    if (table_ && pp.raw == bound_params_ && pk == bound_pk_ && pp.m == bound_m_) return;
    unbind();
    if (pool_) {      // member 0's table is borrowed from the pool table
      if (mp_pool_table_create(pool_, pp.m, pp.n, pp.raw.data(), pk.data(), 0, &ptable_) != MP_OK) throw CardProtocolError(mp_last_error());
      table_ = mp_pool_table_member(ptable_, 0);
    } else if (mp_table_create(ctx_, pp.m, pp.n, pp.raw.data(), pk.data(), &table_) != MP_OK) {
      throw CardProtocolError(mp_last_error());
    }
    bound_params_ = pp.raw;
    bound_pk_ = pk;
    bound_m_ = pp.m;
  }
  void unbind() {
    if (ptable_) mp_pool_table_destroy(ptable_);
    else if (table_) mp_table_destroy(table_);
    ptable_ = nullptr;
    table_ = nullptr;
  }
  int curve_;
  mp_pool* pool_ = nullptr;             // device-list constructor: ctx_ and table_ are member 0's, borrowed
  mp_pool_table* ptable_ = nullptr;
  mp_ctx* ctx_ = nullptr;
  mp_table* table_ = nullptr;
  std::vector<uint8_t> bound_params_;
  PublicKey bound_pk_{};
  uint32_t bound_m_ = 0;
};
typedef DLCardsT<64> DLCards;              // DLCards<starknet_curve / bn254 / secp256k1>
typedef DLCardsT<96> DLCardsBls12_377;     // DLCards<ark_bls12_377::G1Projective> [REF examples/parameter_selection.rs:25-29]
typedef DLCards::PublicKey PublicKey;
typedef DLCards::MaskedCard MaskedCard;

}  // namespace barnett_smart
