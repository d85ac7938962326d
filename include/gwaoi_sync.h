/*
 * gwaoi_sync.h -- entity position sync on the GPU: the callers either side of
 * the AOI path, on the same world and
 * stream as gwaoi.h.
 *
 *   reference (file:line, /root/reference)                      replaced by
 *   ------------------------------------------------------     ------------------------------------
 *   GameService.HandleSyncPositionYawFromClient                 gwaoi_sync_from_clients(_device)
 *     components/game/GameService.go:392-404  (32-B records:
 *     EntityID[16] + x,y,z,yaw float32 little-endian)
 *   entity.OnSyncPositionYawFromClient  EntityManager.go:484-493 (ID lookup; unknown IDs are skipped)
 *   Entity.syncPositionYawFromClient    Entity.go:430-435       (only if SetClientSyncing(true))
 *   Entity.SetClientSyncing             Entity.go:437-440       gwaoi_entity_set_syncing
 *   Entity.setPositionYaw / SetPosition Entity.go:1185-1205     gwaoi_set_position_yaw
 *   Space.enter / Space.leave without AOI (no EnableAOI, or IsUseAOI false)
 *     Space.go:188-251                                        gwaoi_entity_enter_plain / _leave_plain
 *   CollectEntitySyncInfos              Entity.go:1221-1267     gwaoi_collect_sync_infos(_device)
 *     (per-gate MT_SYNC_POSITION_YAW_ON_CLIENTS payloads of 48-B records:
 *      ClientID[16] + EntityID[16] + x,y,z,yaw float32)
 *   Entity.interest / uninterest -> GameClient.sendCreateEntity / sendDestroyEntity
 *     Entity.go:236-246, GameClient.go:37-59                    gwaoi_collect_client_events
 *   Entity.CallAllClients               Entity.go:743-749       gwaoi_collect_broadcast(_device)
 *   Entity.ForAllClients                Entity.go:768-778         (the own client plus the client of
 *   Entity.sendMapAttrChangeToClients / sendMapAttrDelToClients /  every entity in InterestedBy; the
 *     sendMapAttrClearToClients / sendListAttrChangeToClients /    caller attaches the RPC or
 *     sendListAttrPopToClients / sendListAttrAppendToClients       attribute payload per record)
 *     for AllClients attributes         Entity.go:814-917
 *   Entity.SetClient                    Entity.go:678-724       gwaoi_collect_client_switch
 *   Entity.GiveClientTo                 Entity.go:752-765         (the create / destroy lists of the
 *                                                                  entities in InterestedBy, and the switch)
 *   loops over Entity.InterestedIn     examples/unity_demo/Monster.go:49-65 (Monster.AI),
 *     examples/test_game/Avatar.go:281-307                      gwaoi_neighbors_batch(_device)
 *   Entity.IsInterestedIn               Entity.go:248-251       gwaoi_related_batch(_device)
 *     (Monster.Tick, Monster.go:81,91)
 *   Monster.AI's nearest living Player: Entity.DistanceTo       gwaoi_entity_set_tag(_batch) +
 *     Entity.go:253-256, Vector3.go:22-28                         gwaoi_nearest_batch(_device)
 *   Monster.Tick's chase: SetPosition(mypos +                  gwaoi_steer_batch(_device)
 *     Normalized(target - mypos) * step)  examples/unity_demo/Monster.go:80-102
 *   Entity.FaceTo / FaceToPos           Entity.go:1292-1304       (GWAOI_STEER_MOVE, GWAOI_STEER_FACE)
 *     Vector3.DirToYaw / Normalize      Vector3.go:44-77
 *   Monster.AI's range test: DistanceTo(monster) >             gwaoi_range_batch(_device),
 *     GetAttackRange()  examples/unity_demo/Monster.go:72,108     gwaoi_range_count_batch(_device)
 *     and Monster.attack (Monster.go:143-151) for everyone in     (DistanceTo <= r about an entity or
 *     range instead of one player                                   a point)
 *
 * Entity ids and client ids are the reference's 16-byte strings
 * (common.ENTITYID_LENGTH = common.CLIENTID_LENGTH = uuid.UUID_LENGTH = 16,
 * engine/common/types.go:9,46).  The world keeps, per slot: the entity id
 * (device hash table id -> slot, for the packet decode), the client
 * (gate id + client id, or none), the syncing-from-client flag, the last
 * synced position and yaw (AOI itself uses X/Z only), and the sync flags
 * (sifSyncOwnClient / sifSyncNeighborClients, Entity.go:1198-1203).
 *
 * Ordering.  Sync calls share the world's call order: a decoded packet is a
 * device Moved batch queued after everything before it; the last write of a
 * slot's Y/yaw wins exactly as the sequential calls would leave it.
 * gwaoi_collect_* read the state of the last flush (gwaoi_tick*): call them
 * with no queued op (GWAOI_ESTATE otherwise), as GoWorld does (the collect
 * runs after the position packets of the tick have been handled,
 * GameService.go:171-183).
 *
 * Records of one gate come in an unspecified order (the reference iterates Go
 * maps); the multiset per gate is exact.
 */
#ifndef GWAOI_SYNC_H
#define GWAOI_SYNC_H

#include <stddef.h>
#include <stdint.h>

#include "gwaoi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GWAOI_ID_LEN 16          /* EntityID / ClientID bytes                                   */
#define GWAOI_SYNC_IN_REC 32     /* client -> game record: EntityID + x,y,z,yaw                 */
#define GWAOI_SYNC_OUT_REC 48    /* game -> gate record: ClientID + EntityID + x,y,z,yaw        */
#define GWAOI_DESTROY_REC 32     /* game -> gate destroy record: ClientID + EntityID            */
#define GWAOI_MAX_GATES 1024     /* distinct gate ids a world may route to                      */

#define GWAOI_SIF_OWN_CLIENT 1u       /* sifSyncOwnClient       */
#define GWAOI_SIF_NEIGHBOR_CLIENTS 2u /* sifSyncNeighborClients */

/* Per-gate output of a collect: gate g (id gate_ids[g]) owns records
 * [offsets[g], offsets[g+1]).  Host pointers are world-owned and valid until
 * the next collect of the same kind; `records` is host memory for
 * gwaoi_collect_sync_infos and device memory for the _device form. */
typedef struct {
    uint32_t n_gates;
    const uint16_t *gate_ids;
    const uint64_t *offsets;   /* n_gates + 1 entries, in records */
    const uint8_t *records;    /* offsets[n_gates] * record bytes */
} gwaoi_gate_records;

/* ---- per-entity state ---------------------------------------------------- */
/* Bind a slot to its entity id (entity creation).  GWAOI_ESTATE if the id is
 * bound to another slot or the slot to another id. */
int gwaoi_entity_bind(gwaoi_world *w, uint32_t slot, const uint8_t eid[GWAOI_ID_LEN]);
int gwaoi_entity_bind_batch(gwaoi_world *w, const uint32_t *slots, const uint8_t *eids, size_t n);
/* Drop the id of a slot (entity destroyed); also clears its client. */
int gwaoi_entity_unbind(gwaoi_world *w, uint32_t slot);
/* Entity.SetClient: gate id + client id; clientid == NULL clears the client. */
int gwaoi_entity_set_client(gwaoi_world *w, uint32_t slot, uint16_t gate_id, const uint8_t *clientid);
/* Entity.SetClientSyncing. */
int gwaoi_entity_set_syncing(gwaoi_world *w, uint32_t slot, int syncing);
/* Position and yaw of a slot as the sync records report them, without a
 * Moved call or a sync flag (entity creation; before gwaoi_enter, which sets
 * both sync flags as Space.enter does, Space.go:203-205). */
int gwaoi_entity_set_position_yaw(gwaoi_world *w, uint32_t slot, float x, float y, float z, float yaw);

/* Space.enter of a space without AOI (EnableAOI never called), or of an
 * entity type without AOI (IsUseAOI false, Space.go:210): Position = (x,y,z)
 * and both sync flags (Space.go:201-205), no AOI call; the entity has no AOI
 * neighbours there.  GWAOI_ESTATE unless the slot is in nilSpace (neither in
 * an AOI space nor in another space without AOI: Space.go:193-195 panics).
 * gwaoi_enter of a slot in such a space is GWAOI_ESTATE too. */
int gwaoi_entity_enter_plain(gwaoi_world *w, uint32_t slot, float x, float y, float z);
/* Space.leave of that space: back to nilSpace (GWAOI_ESTATE if not in one). */
int gwaoi_entity_leave_plain(gwaoi_world *w, uint32_t slot);

/* ---- moves ---------------------------------------------------------------- */
/* Entity.setPositionYaw(pos, yaw, fromClient=false) (server-side move).  A
 * created entity is never in a nil space: outside every space it is in
 * nilSpace (EntityManager.go:250,293; Space.go:240), so Space.move always
 * runs.  In an AOI space: a Moved(x, z) plus Position and yaw.  In nilSpace
 * or a space without AOI, Space.move returns before Position
 * (Space.go:253-257): only yaw changes.  Both sync flags either way; the
 * own-client record then carries the stale Position with the new yaw. */
int gwaoi_set_position_yaw(gwaoi_world *w, uint32_t slot, float x, float y, float z, float yaw);

/* HandleSyncPositionYawFromClient: decode n_rec 32-B records (host memory)
 * on the GPU into one device Moved batch, in record order.  Records whose
 * id is unknown or whose entity is not syncing from its client are skipped
 * silently, as in the reference.  The others are setPositionYaw(fromClient):
 * in an AOI space a Moved plus Position and yaw, elsewhere yaw only (as
 * above); every applied record raises sifSyncNeighborClients. */
int gwaoi_sync_from_clients(gwaoi_world *w, const uint8_t *payload, size_t n_rec);
/* Same, payload already in device memory of the world's GPU (16-B aligned);
 * it must stay valid until the next gwaoi_tick*. */
int gwaoi_sync_from_clients_device(gwaoi_world *w, const uint8_t *d_payload, size_t n_rec);

/* ---- collect ---------------------------------------------------------------- */
/* CollectEntitySyncInfos: for every flagged entity, a record to its own
 * client (sifSyncOwnClient) and to the client of every entity interested in
 * it (sifSyncNeighborClients, the go-aoi relation of the last flush); then
 * clears every flag.  Records go to host memory. */
int gwaoi_collect_sync_infos(gwaoi_world *w, gwaoi_gate_records *out);
/* Same; records stay in device memory. */
int gwaoi_collect_sync_infos_device(gwaoi_world *w, gwaoi_gate_records *out);
/* The last flush's events routed to clients: enter (a,b) with a client on a
 * -> create record (a's ClientID, b's EntityID, b's x,y,z,yaw: 48 B);
 * leave (a,b) -> destroy record (a's ClientID, b's EntityID: 32 B).  The
 * caller adds type name and client data per record (GameClient.go:37-53).
 * Host memory. */
int gwaoi_collect_client_events(gwaoi_world *w, gwaoi_gate_records *creates, gwaoi_gate_records *destroys);

/* ---- broadcast ------------------------------------------------------------ */
#define GWAOI_CAST_REC 32        /* ClientID[16] | msg u32 | src slot u32 | dst slot u32 | 0 u32, little-endian */
#define GWAOI_CAST_OWN 1u        /* the source's own client (e.client.call / sendNotify*)          */
#define GWAOI_CAST_NEIGHBORS 2u  /* the client of every entity in the source's InterestedBy         */

/* AllClients delivery (CallAllClients, ForAllClients and the AllClients
 * attribute notifications, Entity.go:743-917) of a batch of n messages:
 * per-gate lists of (receiving ClientID, message index).
 *
 * Messages.  Message m is entry m of the arrays; `msg` of a record is m, so
 * the caller attaches the payload.  flags == NULL means OWN | NEIGHBORS for
 * every message.  A slot may appear any number of times: each message fans
 * out on its own.  flags[m] == 0 yields nothing.
 * Relation.  The go-aoi relation of the last committed flush, the one
 * gwaoi_neighbors and gwaoi_collect_sync_infos read: GWAOI_ESTATE with ops
 * queued or a flush in flight, as for the collects.
 * Records.  An OWN record has dst == src and is emitted if the source has a
 * client, whether or not the source is in an AOI space.  A NEIGHBORS record
 * is emitted for each b with rel(src, b) (b in src's InterestedBy) that has a
 * client: dst is b's slot and the record goes to b's gate.  The source never
 * appears as its own neighbour.  (GameClient's methods are no-ops on a nil
 * client, GameClient.go:61-106: entities without a client get nothing.)
 * Sources outside any AOI frame (nilSpace, a space without AOI, a slot never
 * bound or entered) have no neighbours: only the OWN record can result.
 * State.  The call changes nothing: sync flags, positions and the relation
 * are untouched, and calling it twice gives the same multiset.  Records of
 * one gate come in an unspecified order; the multiset per gate is exact.
 * Output.  `out` is filled as for the other collects, with buffers of its
 * own: valid until the next broadcast collect.  n == 0 or no client anywhere
 * gives an empty result and GWAOI_OK; more than 2^32 - 1 records give
 * GWAOI_ECAPACITY.
 * Errors, host form (nothing is produced): null w, out, or slots with n > 0:
 * GWAOI_EINVAL; a flag bit outside OWN | NEIGHBORS: GWAOI_EINVAL; a slot >=
 * max_slots: GWAOI_EBADSLOT.
 * Errors, device form (d_slots / d_flags in device memory of the world's GPU,
 * read before the call returns): an offending message is dropped, the others
 * are delivered in *out, and the call returns GWAOI_EBADSLOT / GWAOI_EINVAL,
 * as the device Moved batches report; the world stays usable. */
int gwaoi_collect_broadcast(gwaoi_world *w, const uint32_t *slots, const uint32_t *flags, size_t n,
                            gwaoi_gate_records *out);
/* Same; messages in device memory, records stay in device memory. */
int gwaoi_collect_broadcast_device(gwaoi_world *w, const uint32_t *d_slots, const uint32_t *d_flags, size_t n,
                                   gwaoi_gate_records *out);

/* ---- client switches ------------------------------------------------------- */
/* Entity.SetClient for a batch of n entities (Entity.go:678-724; GiveClientTo,
 * Entity.go:752-765, is a detach of one entity and an attach of another): the
 * destroy records the old clients and the create records the new clients get
 * for the entities in each source's InterestedBy, per gate, and the switch.
 *
 * Messages.  Message m sets the client of slots[m] to (gate_ids[m],
 * clientids[16m .. 16m+16)).  An all-zero ClientID, or clientids == NULL,
 * means no client (GoWorld ids are 16 printable bytes); gate_ids[m] is then
 * ignored.  gwaoi_entity_set_client is unchanged.  A slot may appear at most
 * once per call: a repeat is GWAOI_EINVAL and the caller splits the batch
 * (with distinct slots the array order is irrelevant).
 * Old client.  Read from the world's state on the device: every earlier
 * gwaoi_entity_set_client is visible (the call pushes the pending host writes
 * first, as the collects do).
 * No-op.  A message whose new (gate, ClientID) equals the current one, or that
 * detaches an entity without a client, yields nothing (the reference's
 * `oldClient == client` return).
 * Destroy records (GWAOI_DESTROY_REC, 32 B: old ClientID, neighbour EntityID):
 * one per b with rel(src, b) (b in src's InterestedBy), under the old client's
 * gate; only if there was an old client.
 * Create records (GWAOI_SYNC_OUT_REC, 48 B: new ClientID, neighbour EntityID,
 * b's x, y, z, yaw): one per b with rel(src, b), under the new client's gate;
 * only if there is a new client.  x and z are the frame's, y and yaw the
 * slot's position record: exactly gwaoi_collect_client_events' create record.
 * Neighbours.  Whether b has a client is irrelevant; the source is never its
 * own neighbour.
 * What the caller still sends itself.  The entity's own create (isPlayer), its
 * own destroy and the Space entity's record (Entity.go:692-708) are host
 * state.  On a client the order is: all destroy records of the call, then the
 * caller's own / space records, then all create records; that keeps the
 * reference's order per client.
 * Relation.  That of the last committed flush: GWAOI_ESTATE with ops queued or
 * a flush in flight, as for the collects.
 * Sources outside the frame (nilSpace, a space without AOI, a slot never bound
 * or entered) produce no records; their client is still switched.
 * State.  After the call each slot's gate and ClientID are what n
 * gwaoi_entity_set_client calls would have left (gate ids not seen before are
 * registered).  Sync flags, positions and the relation are untouched.
 * Output.  Both results are filled as for the other collects, with buffers of
 * their own: valid until the next switch collect.  Records are in host memory,
 * in an unspecified order within a gate; the multiset per gate is exact.
 * n == 0 gives two empty results and GWAOI_OK.  More than 2^32 - 1 records of
 * either kind (the two share one 32-bit index space: or of both together)
 * give GWAOI_ECAPACITY.
 * Errors.  On any error nothing is produced and nothing is changed.  Null w,
 * creates or destroys, or null slots / gate_ids with n > 0: GWAOI_EINVAL; a
 * slot >= max_slots: GWAOI_EBADSLOT; a repeated slot: GWAOI_EINVAL; a batch
 * that would take the world past GWAOI_MAX_GATES distinct gates:
 * GWAOI_ECAPACITY, checked before any gate is registered. */
int gwaoi_collect_client_switch(gwaoi_world *w, const uint32_t *slots, const uint16_t *gate_ids,
                                const uint8_t *clientids /* 16 B per message, NULL: all detach */,
                                size_t n, gwaoi_gate_records *creates, gwaoi_gate_records *destroys);

/* ---- interest-set reads ---------------------------------------------------- */
/* InterestedIn / InterestedBy as game logic reads them, for a batch of queries
 * on the GPU: the rows themselves, membership of a pair, and the nearest
 * neighbour that passes a tag filter (Monster.AI, Monster.Tick,
 * Avatar.TestCallAll_Client; see the table at the top).
 *
 * Relation.  That of the last committed flush, the one gwaoi_neighbors and the
 * collects read.  Every call below returns GWAOI_ESTATE with ops queued or a
 * flush in flight, exactly as the collects do (a decoded sync packet writes Y
 * and yaw before its flush: a read with ops queued would mix frames).
 * No side effects.  Nothing here changes sync flags, positions, clients or
 * the relation; a query made twice gives the same answer.
 * Outside the frame.  A slot never entered, one that left, one in nilSpace or
 * in a space without AOI has no neighbours: an empty row, membership 0, no
 * nearest.  That is not an error (gwaoi_neighbors keeps its GWAOI_ESTATE).
 * Errors, host forms (nothing is produced): a null world or output, or a null
 * input array with n > 0: GWAOI_EINVAL; a slot >= max_slots: GWAOI_EBADSLOT.
 * Errors, device forms (inputs in device memory of the world's GPU, read
 * before the call returns): a query with a slot >= max_slots gets the
 * "outside the frame" answer, the other answers are delivered, the call
 * returns GWAOI_EBADSLOT and the world stays usable (the broadcast's
 * device-form convention). */

/* Rows of neighbour slots: row m = items[offsets[m] .. offsets[m+1]). */
typedef struct {
    uint32_t n;              /* rows = queries                                   */
    const uint32_t *offsets; /* n + 1 entries; row m = items[offsets[m] .. offsets[m+1]) */
    const uint32_t *items;   /* neighbour slots                                  */
} gwaoi_slot_rows;

/* Row m is InterestedIn of slots[m]; as a set that equals InterestedBy:
 * {b : rel(slots[m], b)}, never the slot itself.  The order within a row is
 * unspecified, the set is exact.  A slot may repeat: each query gets its own
 * row.  offsets and items are world-owned host memory, valid until the next
 * rows call (of either form).  n == 0 gives out->n == 0, a one-entry offsets
 * and GWAOI_OK; more than 2^32 - 1 items give GWAOI_ECAPACITY.
 * These two calls and the membership calls read only the frame: they work on
 * a world on which no other call of this header was ever made, and leave it
 * so (a strip world stays one that accepts device Enter / Leave batches). */
int gwaoi_neighbors_batch(gwaoi_world *w, const uint32_t *slots, size_t n, gwaoi_slot_rows *out);
/* Same; d_slots in device memory, offsets and items both stay in device
 * memory (offsets[n], the number of items, included), valid until the next
 * rows call.  One host wait unless the items outgrew the last call's. */
int gwaoi_neighbors_batch_device(gwaoi_world *w, const uint32_t *d_slots, size_t n, gwaoi_slot_rows *out);

/* out[m] = a[m].IsInterestedIn(b[m]) (Entity.go:248-251): 1 iff both slots are
 * in the frame, in the same space, distinct, and rel() holds for the pair (the
 * owner of the window is the later seq, as everywhere); otherwise 0. */
int gwaoi_related_batch(gwaoi_world *w, const uint32_t *a, const uint32_t *b, size_t n, uint8_t *out);
/* Same; d_a, d_b and d_out (n bytes) in device memory, complete on return. */
int gwaoi_related_batch_device(gwaoi_world *w, const uint32_t *d_a, const uint32_t *d_b, size_t n, uint8_t *d_out);

/* A tag: 32 caller-defined bits per slot (for unity_demo: the entity type and
 * an "hp > 0" bit), 0 by default, kept across Enter / Leave and cleared by
 * gwaoi_entity_unbind.  Setting one is not an AOI op: it is allowed with ops
 * queued and visible to every later query, as gwaoi_entity_set_client is to
 * the collects.  Within one batch the last write of a slot wins.
 * GWAOI_EBADSLOT for a slot >= max_slots (the batch then sets nothing). */
int gwaoi_entity_set_tag(gwaoi_world *w, uint32_t slot, uint32_t tag);
int gwaoi_entity_set_tag_batch(gwaoi_world *w, const uint32_t *slots, const uint32_t *tags, size_t n);

#define GWAOI_NO_SLOT 0xFFFFFFFFu
/* Monster.AI's search (Monster.go:49-65): among the b in InterestedIn(slots[m])
 * with (tag[b] & masks[m]) == wants[m], the one with the smallest squared
 * distance; ties go to the smallest slot.  masks == NULL (wants is then
 * ignored) means every neighbour.
 * Distance.  Vector3.DistanceTo on amd64 (Entity.go:253-256, Vector3.go:22-28):
 * dx = b.x - a.x, likewise dy and dz, d2 = fl32(fl32(fl32(dx*dx) + fl32(dy*dy))
 * + fl32(dz*dz)) with no fused step, out_dist[m] = (float)sqrt((double)d2).
 * x and z are the frame's (the AOI position of the last flush), y is the
 * slot's position record (what the sync records report).  Minimising
 * (d2, slot) picks an entity of minimal DistanceTo: one of the outcomes the
 * reference's map-order loop can produce, and the deterministic one.
 * No candidate (nobody passes the filter, an empty row, a source outside the
 * frame): out_slot[m] = GWAOI_NO_SLOT and out_dist[m] = +inf. */
int gwaoi_nearest_batch(gwaoi_world *w, const uint32_t *slots, const uint32_t *masks, const uint32_t *wants,
                        size_t n, uint32_t *out_slot, float *out_dist);
/* Same; every array in device memory, the outputs complete on return. */
int gwaoi_nearest_batch_device(gwaoi_world *w, const uint32_t *d_slots, const uint32_t *d_masks,
                               const uint32_t *d_wants, size_t n, uint32_t *d_out_slot, float *d_out_dist);

/* ---- range reads ------------------------------------------------------------ */
/* The entities within a caller-chosen radius of an entity or of a point, for a batch of queries on
 * the GPU: an area attack about a monster (Monster.attack, Monster.go:143-151, hits one player
 * inside GetAttackRange() = 3, Monster.go:72,108; this is everyone inside it), an aggro radius
 * smaller than the AOI distance, a trigger zone about a point where nobody stands, a count of
 * players within r.  (TODO.md:19 asks for distances other than the space's one; this is the read,
 * the relation itself keeps the space's distance.)
 *
 * Candidates.  Every entity of the frame of the last committed flush that is in the query's space:
 * the centre slot's space, or `center` itself with GWAOI_RANGE_POINT.  The go-aoi relation plays no
 * part: an entity three AOI distances away is found if the radius reaches it.  A slot-centred query
 * never has its centre in its row; a point query has an entity standing exactly on the point in its
 * row.  Entities in nilSpace or in a space without AOI are not in the frame and are never found.  A
 * slot-centred query whose centre is outside the frame (never entered, left, nilSpace, a space
 * without AOI) has an empty row; that is not an error, as for gwaoi_neighbors_batch.  A space
 * created since the last flush has nobody in the frame: an empty row.
 * Distance.  Vector3.DistanceTo exactly as gwaoi_nearest_batch defines it: dx = b.x - c.x, likewise
 * dy and dz, d2 = fl32(fl32(fl32(dx*dx) + fl32(dy*dy)) + fl32(dz*dz)), no fused step, denormals
 * kept, dist = (float)sqrt((double)d2).  A candidate's x and z are the frame's, its y the slot's
 * position record.  Without POINT the centre's x and z are its frame record and its y its slot
 * record; with POINT the centre is (x, y, z) of the query.  With GWAOI_RANGE_PLANAR the dy*dy term
 * is left out: d2 = fl32(fl32(dx*dx) + fl32(dz*dz)), a cylinder.
 * Hit.  A candidate is a hit iff dist <= radius, compared in float32 (Go's e.DistanceTo(o) <= r:
 * the bound is inclusive), and (tag[b] & mask) == want (gwaoi_entity_set_tag; mask = want = 0:
 * everyone).  dists[] holds that dist.
 * Order.  The order within a row is unspecified, as for gwaoi_neighbors_batch; the set and every
 * distance are exact.  items and dists are parallel.
 * Count.  The _count_ forms give counts[m] = offsets[m+1] - offsets[m] and run the count pass only.
 * State.  GWAOI_ESTATE with ops queued or a flush in flight, as for the interest-set reads.  No side
 * effects: a query made twice gives the same answer.  offsets, items and dists are world-owned and
 * valid until the next range call (of either form).  n == 0 gives out->n == 0, a
 * one-entry offsets and GWAOI_OK.  More than 2^32 - 1 items give GWAOI_ECAPACITY.
 * Errors, host forms (nothing is produced, everything is checked before any device work): a null
 * world or output, or a null query array with n > 0: GWAOI_EINVAL; a flag bit outside the two:
 * GWAOI_EINVAL; radius < 0: GWAOI_EINVAL (-0.0 is 0); a NaN or infinite radius: GWAOI_ENONFINITE; a
 * NaN or infinite point coordinate with POINT: GWAOI_ENONFINITE; a slot >= max_slots:
 * GWAOI_EBADSLOT; an unknown or destroyed space with POINT: GWAOI_EBADSPACE (a valid space with
 * nobody in it gives an empty row and GWAOI_OK).
 * Errors, device forms (d_q in device memory of the world's GPU, 16-B aligned, read before the call
 * returns; a misaligned d_q is GWAOI_EINVAL): the offending query gets an empty row (count 0),
 * every other answer is delivered, the world stays usable and the call returns the matching code
 * (the broadcast's device-form convention).  A space id >= max_spaces is the only bad space the
 * device sees; an id below it that names no space has nobody in it.  When several classes occur in
 * one call, the code of any one of them comes back.
 * Cost.  One wave per query; the time follows the candidates in the cells the radius covers.  A
 * radius that spans a whole large space is correct and slow. */
#define GWAOI_RANGE_POINT  1u  /* center is a space id, (x, y, z) the centre; else center is a slot */
#define GWAOI_RANGE_PLANAR 2u  /* drop dy: d2 = fl32(fl32(dx*dx) + fl32(dz*dz)) (a cylinder) */

typedef struct {          /* 32 B */
    uint32_t center;      /* slot, or space id with GWAOI_RANGE_POINT */
    uint32_t flags;
    float x, y, z;        /* the point; ignored without GWAOI_RANGE_POINT */
    float radius;
    uint32_t mask, want;  /* a hit also needs (tag[b] & mask) == want; 0, 0: everyone */
} gwaoi_range_query;

typedef struct {
    uint32_t n;
    const uint32_t *offsets; /* n + 1 entries; row m = items[offsets[m] .. offsets[m+1]) */
    const uint32_t *items;   /* slots */
    const float *dists;      /* parallel to items */
} gwaoi_range_rows;

int gwaoi_range_batch(gwaoi_world *w, const gwaoi_range_query *q, size_t n, gwaoi_range_rows *out);
/* Same; d_q in device memory, offsets, items and dists stay in device memory (offsets[n], the
 * number of items, included).  One host wait unless the items outgrew the last call's. */
int gwaoi_range_batch_device(gwaoi_world *w, const gwaoi_range_query *d_q, size_t n, gwaoi_range_rows *out);
/* out_counts[m] = the length of row m (n entries of the caller's). */
int gwaoi_range_count_batch(gwaoi_world *w, const gwaoi_range_query *q, size_t n, uint32_t *out_counts);
/* Same; d_q and d_out_counts in device memory, complete on return. */
int gwaoi_range_count_batch_device(gwaoi_world *w, const gwaoi_range_query *d_q, size_t n, uint32_t *d_out_counts);

/* ---- server-driven movement ------------------------------------------------- */
/* Monster.Tick's step for a batch of n entities (Monster.go:80-102): move toward a target and face
 * it, on the GPU, from the positions the device already holds.  With gwaoi_nearest_batch_device
 * giving the targets (the IsInterestedIn gate is part of this call) the whole NPC step needs no
 * position on the host: nearest -> steer -> flush -> collect.
 *
 * Messages.  Message m is (movers[m], targets[m], steps[m], flags[m]); flags == NULL means
 * MOVE | FACE for every message.
 * Gate.  A message applies iff flags[m] != 0 and movers[m].IsInterestedIn(targets[m]) on the
 * relation of the last committed flush: exactly gwaoi_related_batch's answer for the pair (both
 * branches of Monster.Tick test it, Monster.go:81,91).  A message that does not apply gets
 * out_applied[m] = 0 and four zero words in out_pos, changes nothing and is not an error: a mover or
 * target outside the frame, in another space or never bound, mover == target, and targets[m] ==
 * GWAOI_NO_SLOT, so that gwaoi_nearest_batch_device's output can be passed on as it is.
 * Snapshot.  Every message reads the state before the call: x and z of both entities from the frame
 * (the AOI position of the last flush, gwaoi_nearest_batch's convention), the mover's y and yaw from
 * its slot record.  A target that is itself a mover of the batch is seen at its old position.
 * Arithmetic.  The reference's on amd64, float32 step by step, nothing fused, IEEE division,
 * denormals kept.  a is the mover, b the target, s = steps[m].
 *   MOVE: dx = b.x - a.x, dy = 0, dz = b.z - a.z; Vector3.Normalize as written (Vector3.go:64-72):
 *   d = (float)sqrt((double)(dx*dx + dy + dy + dz*dz)), the sum taken left to right; d == 0 leaves
 *   the direction as it is (also when dx*dx underflowed to zero with dx != 0), otherwise each
 *   component is divided by d.  Position' = (a.x + nx*s, a.y + ny*s, a.z + nz*s).  The effect is
 *   setPositionYaw(Position', yaw unchanged, fromClient = false): a Moved(x', z'), Position and both
 *   sync flags.
 *   FACE: after the move, from the new position: dx = b.x - x', dz = b.z - z', the same Normalize,
 *   then Vector3.DirToYaw (Vector3.go:45-62) in float64: acos(X), 2 pi - yaw if Z < 0, / pi * 180,
 *   yaw <= 90 ? 90 - yaw : 90 + (360 - yaw), cast to float32.  The effect is SetYaw: yaw and both
 *   sync flags.
 *   |X| <= 1 whenever fl(dx*dx) is a normal float32, zero or +inf: d >= fl(sqrt(fl(dx*dx))) = |dx|
 *   by monotonicity (a sum that overflows gives d = +inf and the direction (0, 0, 0)), so no NaN
 *   arises from such coordinates.  The one exception is the reference's own: for 1.1e-19 > |dx| >
 *   2.6e-23 the square is a denormal with fewer than 24 bits, it may round down, and then d < |dx|
 *   and X slightly above 1 (1.0097 for dx = 1e-22, dz = 0): acos(X) is NaN there in the reference
 *   too, and X * step can overflow for a step near the largest float32.
 * Yaw is not bit-exact.  Positions are the reference's bit for bit; yaw goes through a float64 acos
 * that is not the Go runtime's: it equals the reference's to within one float32 ulp (as an angle,
 * modulo 360: DirToYaw jumps from 0 to 360 at yaw = 90).
 * out_applied[m] is 1 iff message m applied; out_pos[4m .. 4m+4) is the mover's x, y, z, yaw after it.
 * Order.  The applied MOVE messages are one device Moved batch in message order, queued after
 * everything before it as a decoded packet is; Position and yaw take last-writer claims like every
 * other write, so a later gwaoi_set_position_yaw or packet for the same slot in the same flush wins,
 * as the sequential calls would leave it.
 * State.  GWAOI_ESTATE with ops queued or a flush in flight, as for the reads: the call needs the
 * relation and the frame of one flush.  A call with n > 0 counts as a queued op: flush before the
 * next read, collect or steer (one steer call per loop iteration, holding every entity whose Tick
 * fires in it).
 * Movers are distinct (each message would have to read what the previous one wrote); targets may
 * repeat freely.  Host form: a repeated mover is GWAOI_EINVAL and nothing happens.  Device form: one
 * message of a repeated mover applies (which one is unspecified), the others are dropped with
 * out_applied = 0, and the call returns GWAOI_EINVAL.
 * Errors, host form (before any device work, nothing changed): null w, or a null array other than
 * flags with n > 0: GWAOI_EINVAL; a flag bit outside MOVE | FACE: GWAOI_EINVAL; a mover >= max_slots
 * or a target >= max_slots other than GWAOI_NO_SLOT: GWAOI_EBADSLOT; a non-finite step:
 * GWAOI_ENONFINITE.
 * Errors, device form (every array in device memory of the world's GPU, the outputs complete on
 * return): an offending message is dropped (out_applied = 0), the others are delivered and the call
 * returns the code; of several, GWAOI_EBADSLOT, then GWAOI_EINVAL, then GWAOI_ENONFINITE.
 * Both forms: a message whose new x or z is not finite, or whose yaw is NaN (the exception above;
 * where the reference would go on with a NaN yaw or an infinite Position), is dropped the same way
 * and the call returns GWAOI_ENONFINITE, the host form with the other answers delivered; the slot
 * record never holds a position the flush would refuse.  The world stays usable after every error. */
#define GWAOI_STEER_MOVE 1u   /* Monster.go:92-97: SetPosition(mypos + Normalized(dir) * step)      */
#define GWAOI_STEER_FACE 2u   /* Entity.FaceTo(target), Entity.go:1292-1304 (after the move, if both) */

int gwaoi_steer_batch(gwaoi_world *w, const uint32_t *movers, const uint32_t *targets, const float *steps,
                      const uint32_t *flags /* NULL: MOVE | FACE */, size_t n,
                      uint8_t *out_applied /* n */, float *out_pos /* 4n: x, y, z, yaw */);
/* Same; every array in device memory of the world's GPU. */
int gwaoi_steer_batch_device(gwaoi_world *w, const uint32_t *d_movers, const uint32_t *d_targets,
                             const float *d_steps, const uint32_t *d_flags /* NULL: MOVE | FACE */, size_t n,
                             uint8_t *d_out_applied, float *d_out_pos);

#ifdef __cplusplus
}
#endif

#endif /* GWAOI_SYNC_H */
